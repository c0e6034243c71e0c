// Training-data transforms (reference climategan/transforms.py:22-289, 424-490): the loaders' hflip / resize / crop / resize
// pipeline, Normalize and BucketizeDepth as ONE gather per task and batch, and the pipeline's colour jitter.
//   cgan_data_transform   sample k: source map of its own size -> dense [C][out_h][out_w] at its own dst.  The host reduces any
//                         sequence of flips, crops and resizes to at most two resampling stages with an integer index map
//                         before, between and after them (include/climategan_hip.h); the kernel walks that plan backwards
//                         from the output pixel and touches only the source pixels the final window needs.
//                         With a raw source kind (nearest mode) tensor_loader's decode (data.py:91-148, 231-252, 344-399;
//                         tutils.py:195-293) is applied to the gathered pixel before the store, so that a 160 x 160 task
//                         decodes 1 % of a 1200 x 1800 source and the upload is the file's own bytes.
//   cgan_data_source_minmax  the one thing that has to see the whole source: min / max for the normalised depth modes, x and
//                         the mask's "max > 127", as fixed-range partials over 16-byte non-temporal loads and a fixed-order
//                         finish that leaves (min, range, max, flag) where the gather's items point.
//   cgan_data_jitter      brightness / saturation / contrast of the final-size x (transforms.py:494-541, the
//                         is_diff_augment=False branches, bound to torchvision's documented formulas), the dummy pixels and,
//                         on the last item, Normalize.
// The index arithmetic is ATen's own, in fp32 (ATen/native/UpSample.h):
//   nearest   nearest_idx -> nearest_neighbor_compute_source_index: min((int64)floorf(dst * scale), in - 1) with
//             scale = compute_scales_value = (float)in / out
//   bilinear  area_pixel_compute_scale (align_corners): (float)(in - 1) / (out - 1), 0 when out == 1;
//             area_pixel_compute_source_index (align_corners): scale * dst; guard_index_and_lambda: i0 = min((int64)floorf(src),
//             in - 1), lambda = clamp(src - i0, 0, 1); i1 = min(i0 + 1, in - 1); weights 1 - lambda, lambda
// so the weights equal the reference's bit for bit; float64 index arithmetic is off by 1e-4 on x.  No contraction anywhere
// in this file: a fused multiply-add in `scale * dst` followed by `- i0` would change lambda.
// Memory-bound gathers: 32-bit offsets inside a sample, every load of a thread issued before its first use (16 taps x C for
// x, four pixels per thread for the one-tap maps), non-temporal stores (the output is written once and read by a later
// launch at the earliest).  No atomics, no LDS outside the contrast reduction.
#include "cgan_common.h"

#include <type_traits>

#pragma clang fp contract(off)

namespace {

constexpr int kParts = CGAN_DIFFAUG_PARTS;

struct Affine4 {
  float mean[4], std[4];
};

__device__ __forceinline__ int map_col(const CganDataTfMap& m, int j) { return m.flip ? m.col_off - j : m.col_off + j; }

__device__ __forceinline__ int near_idx(int dst, int in, int out) {
  return nearest_src(dst, (float)in / (float)out, in);   // cgan_common.h: min((int)floorf(dst * scale), in - 1)
}

__device__ __forceinline__ void bil_axis(int dst, int in, int out, int& i0, int& i1, float& lam) {
  const float scale = out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  const float src = scale * (float)dst;
  const int f = (int)floorf(src);
  i0 = f < in - 1 ? f : in - 1;
  lam = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
  i1 = i0 + 1 < in - 1 ? i0 + 1 : in - 1;
}

// ATen's order (UpSampleKernel.cpp, Interpolate<2>): rows outside, columns inside
__device__ __forceinline__ float bil4(float ly, float lx, float v00, float v01, float v10, float v11) {
  const float wy0 = 1.f - ly, wx0 = 1.f - lx;
  return wy0 * (wx0 * v00 + lx * v01) + ly * (wx0 * v10 + lx * v11);
}

// ------------------------------------------------------------------------------------------------ nearest
// source element offset of output pixel (oy, ox)
template <int NS>
__device__ __forceinline__ int near_offset(const CganDataTfItem& it, int oy, int ox) {
  int y = it.map[NS].row_off + oy, x = map_col(it.map[NS], ox);
#pragma unroll
  for (int k = NS - 1; k >= 0; --k) {
    y = it.map[k].row_off + near_idx(y, it.stage[k].in_h, it.stage[k].out_h);
    x = map_col(it.map[k], near_idx(x, it.stage[k].in_w, it.stage[k].out_w));
  }
  return y * it.stride_h + x * it.stride_w;
}

// torch.bucketize(v, boundaries, right=True): the first index whose boundary is greater than v (ATen Bucketization.cpp,
// cus_upper_bound: the same loop, so that a NaN lands where ATen puts it)
__device__ __forceinline__ int bucket_of(float v, const float* __restrict__ b, int n) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (!(b[mid] > v)) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ------------------------------------------------------------------------------------------------ raw sources
// The decode of one gathered pixel.  fp32 division, multiplication and reciprocal are the IEEE operations (contraction is off
// and nothing here is built with fast-math); the integer parts are exact.
__device__ __forceinline__ float unity_depth(int r, int g, int b, float far_plane) {
  // tutils.py:276-280: ((247 - R) / 8).type(IntTensor) truncates toward zero like C's int division: 248..254 -> 0, 255 -> -1
  const int code = ((247 - r) / 8) * (256 * 31) + ((247 - g) / 8) * 256 + (255 - b);
  return (float)code / 246015.f * far_plane;
}
__device__ __forceinline__ float kitti_depth(uint32_t v) { return (float)v / 100.f; }   // tutils.py:208

// log in float64 on the fp32 depth, rounded once more to fp32: correctly rounded up to double rounding
__device__ __forceinline__ float log_f32(float d) { return (float)log((double)d); }

// NaN wins, as in torch.min / torch.max
__device__ __forceinline__ float nan_min(float a, float b) { return a != a ? a : (b != b ? b : (b < a ? b : a)); }
__device__ __forceinline__ float nan_max(float a, float b) { return a != a ? a : (b != b ? b : (b > a ? b : a)); }

template <int KIND>
__device__ __forceinline__ uint32_t load_raw(const void* src, int off, int sc) {
  if constexpr (KIND == CGAN_DTF_SRC_KITTI_D) {
    return reinterpret_cast<const uint16_t*>(src)[off];
  } else if constexpr (KIND == CGAN_DTF_SRC_F32_D) {
    return reinterpret_cast<const uint32_t*>(src)[off];
  } else {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(src) + off;
    uint32_t v = p[0];
    if constexpr (KIND != CGAN_DTF_SRC_MASK) v |= (uint32_t)p[sc] << 8 | (uint32_t)p[2 * sc] << 16;
    if constexpr (KIND == CGAN_DTF_SRC_SEG_NEAREST) v |= (uint32_t)p[3 * sc] << 24;
    return v;
  }
}

struct RawConsts {
  float mn, rng, far_plane;
  int flags;
};

template <int KIND>
__device__ __forceinline__ float decode_raw(uint32_t raw, const RawConsts& k, const CganDataTfPalette& pal) {
  if constexpr (KIND == CGAN_DTF_SRC_UNITY_D || KIND == CGAN_DTF_SRC_KITTI_D) {
    const float depth = KIND == CGAN_DTF_SRC_UNITY_D
                            ? unity_depth(raw & 255, (raw >> 8) & 255, (raw >> 16) & 255, k.far_plane)
                            : kitti_depth(raw);
    if (k.flags & CGAN_DTF_DEC_LOG) return log_f32(depth);
    const float inv = 1.f / depth;
    return (k.flags & CGAN_DTF_DEC_NORMALIZE) ? (inv - k.mn) / k.rng : inv;
  } else if constexpr (KIND == CGAN_DTF_SRC_F32_D) {
    return (__builtin_bit_cast(float, raw) - k.mn) / k.rng;               // tutils.py:199-201
  } else if constexpr (KIND == CGAN_DTF_SRC_MASK) {
    return (k.flags & CGAN_DTF_DEC_THRESHOLD) ? (raw > 127u ? 1.f : 0.f) : (float)raw;   // data.py:392-393
  } else if constexpr (KIND == CGAN_DTF_SRC_SEG_EXACT) {
    int cls = pal.default_class;                                          // data.py:104-107, 123-126
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (i < pal.n && raw == pal.colour[i]) cls = pal.cls[i];
    return (float)cls;
  } else {
    int best = 0x7fffffff, cls = 0;                                       // data.py:221-228: strict <, the first wins
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i < pal.n) {
        const uint32_t c = pal.colour[i];
        const int d0 = (int)(raw & 255) - (int)(c & 255), d1 = (int)((raw >> 8) & 255) - (int)((c >> 8) & 255);
        const int d2 = (int)((raw >> 16) & 255) - (int)((c >> 16) & 255), d3 = (int)(raw >> 24) - (int)(c >> 24);
        const int d = d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        if (d < best) best = d, cls = pal.cls[i];
      }
    }
    return (float)cls;
  }
}

// ------------------------------------------------------------------------------------------------ the nearest gather
// The source policy is KIND: CGAN_DTF_SRC_B4 / B8 gather every channel's 4- or 8-byte element as it is; a raw kind reads one
// pixel (all the channels of its code) and writes the one channel it decodes to.
template <int KIND>
struct NearSource {
  static constexpr bool kRaw = KIND >= CGAN_DTF_SRC_UNITY_D;
  using Elem = std::conditional_t<KIND == CGAN_DTF_SRC_B8, uint64_t, uint32_t>;
  static __device__ __forceinline__ int channels(const CganDataTfItem& it) { return kRaw ? 1 : it.channels; }
  static __device__ __forceinline__ Elem load(const CganDataTfItem& it, int off, int c) {
    if constexpr (kRaw) return load_raw<KIND>(it.src, off, it.stride_c);
    else return reinterpret_cast<const Elem*>(it.src)[c * it.stride_c + off];
  }
};

constexpr int kNearPix = 4;   // output pixels per thread: that many loads in flight

template <int KIND, int NS, bool BUCKET>
__global__ __launch_bounds__(256) void data_tf_nearest_kernel(const CganDataTfItem* __restrict__ items,
                                                              const float* __restrict__ bounds, int n_bounds,
                                                              CganDataTfPalette pal) {
  using S = NearSource<KIND>;
  using E = typename S::Elem;
  const CganDataTfItem it = items[blockIdx.y];
  const int ohw = it.out_h * it.out_w;
  const int p0 = blockIdx.x * (256 * kNearPix) + threadIdx.x;
  if (p0 >= ohw) return;
  int off[kNearPix];
  E v[kNearPix];
#pragma unroll
  for (int k = 0; k < kNearPix; ++k) {
    const int p = p0 + k * 256;
    const int pc = p < ohw ? p : p0;          // a thread past the end repeats its first pixel and does not store
    const int oy = pc / it.out_w, ox = pc - oy * it.out_w;
    off[k] = near_offset<NS>(it, oy, ox);
    // a raw kind's one pixel is loaded next to its offset: its 3 or 4 byte addresses die before the next pixel's are formed
    // (2 VGPRs less for the SEG kinds than loading after the loop)
    if constexpr (S::kRaw) v[k] = S::load(it, off[k], 0);
  }
  RawConsts kc = {it.u8_min, it.u8_range, it.far_plane, it.dec_flags};
  if (S::kRaw && it.stats) {   // written by cgan_data_source_minmax earlier on this stream
    kc.mn = it.stats[0], kc.rng = it.stats[1];
    kc.flags = (kc.flags & ~CGAN_DTF_DEC_THRESHOLD) | (it.stats[3] != 0.f ? CGAN_DTF_DEC_THRESHOLD : 0);
  }
  for (int c = 0; c < S::channels(it); ++c) {
    if constexpr (!S::kRaw) {
#pragma unroll
      for (int k = 0; k < kNearPix; ++k) v[k] = S::load(it, off[k], c);
    }
#pragma unroll
    for (int k = 0; k < kNearPix; ++k) {
      const int p = p0 + k * 256, o = c * ohw + p;
      if (p >= ohw) continue;
      if constexpr (!S::kRaw && !BUCKET) {
        CGAN_ST_STREAM(v[k], reinterpret_cast<E*>(it.dst) + o);
      } else {
        float f;
        if constexpr (S::kRaw) f = decode_raw<KIND>(v[k], kc, pal);
        else f = __builtin_bit_cast(float, v[k]);
        if constexpr (BUCKET) {
          CGAN_ST_STREAM((int32_t)bucket_of(f, bounds, n_bounds), reinterpret_cast<int32_t*>(it.dst) + o);
        } else if constexpr (KIND == CGAN_DTF_SRC_SEG_EXACT) {
          CGAN_ST_STREAM((double)f, reinterpret_cast<double*>(it.dst) + o);   // torch.tensor(np.ones(...) * 14): float64
        } else {
          CGAN_ST_STREAM(f, reinterpret_cast<float*>(it.dst) + o);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ whole-source min / max
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// a group = 16 bytes of a one-value-per-element source, or 16 pixels (CH x 16 bytes) of a Unity depth code
template <int KIND, int CH>
struct MinmaxGroup {
  static constexpr int kLoads = KIND == CGAN_DTF_SRC_UNITY_D ? CH : 1;
  static constexpr int kUnits = KIND == CGAN_DTF_SRC_KITTI_D ? 8 : (KIND == CGAN_DTF_SRC_F32_D ? 4 : 16);
  static constexpr int kUnitBytes = KIND == CGAN_DTF_SRC_UNITY_D ? CH : 16 / kUnits;
};

// number of units of a sample: pixels, or bytes for the kinds that look at every channel
template <int KIND>
__device__ __forceinline__ long minmax_units(const CganDataMinmaxItem& it) {
  return (KIND == CGAN_DTF_SRC_U8 || KIND == CGAN_DTF_SRC_MASK) ? it.pixels * it.channels : it.pixels;
}

__host__ __device__ inline int minmax_parts(long groups) {
  const long p = (groups + 1023) / 1024;   // about four groups per thread
  return (int)(p < 1 ? 1 : (p > kParts ? kParts : p));
}

template <int KIND>
__device__ __forceinline__ float minmax_value(uint32_t raw, float far_plane) {
  if constexpr (KIND == CGAN_DTF_SRC_UNITY_D)
    return 1.f / unity_depth(raw & 255, (raw >> 8) & 255, (raw >> 16) & 255, far_plane);
  else if constexpr (KIND == CGAN_DTF_SRC_KITTI_D) return 1.f / kitti_depth(raw);
  else if constexpr (KIND == CGAN_DTF_SRC_F32_D) return __builtin_bit_cast(float, raw);
  else return (float)raw;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t* w, int k) { return (w[k >> 2] >> ((k & 3) * 8)) & 255u; }

__device__ inline void block_minmax256(float& mn, float& mx, float* sh) {
  sh[threadIdx.x] = mn, sh[256 + threadIdx.x] = mx;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh[threadIdx.x] = nan_min(sh[threadIdx.x], sh[threadIdx.x + s]);
      sh[256 + threadIdx.x] = nan_max(sh[256 + threadIdx.x], sh[256 + threadIdx.x + s]);
    }
    __syncthreads();
  }
  mn = sh[0], mx = sh[256];
}

template <int KIND, int CH>
__global__ __launch_bounds__(256) void minmax_partial_kernel(const CganDataMinmaxItem* __restrict__ items,
                                                             float* __restrict__ ws) {
  using G = MinmaxGroup<KIND, CH>;
  __shared__ float sh[512];
  const CganDataMinmaxItem it = items[blockIdx.y];
  const long units = minmax_units<KIND>(it), groups = units / G::kUnits;
  const int parts = minmax_parts(groups);
  if ((int)blockIdx.x >= parts) return;
  const long chunk = (groups + parts - 1) / parts;
  const long lo = blockIdx.x * chunk, hi = lo + chunk < groups ? lo + chunk : groups;
  float mn = __builtin_inff(), mx = -__builtin_inff();
  const u32x4* src = reinterpret_cast<const u32x4*>(it.src);
  for (long g = lo + threadIdx.x; g < hi; g += 256) {
    uint32_t w[4 * G::kLoads];
#pragma unroll
    for (int j = 0; j < G::kLoads; ++j) {
      const u32x4 q = CGAN_LD_STREAM(src + g * G::kLoads + j);
      w[4 * j] = q.x, w[4 * j + 1] = q.y, w[4 * j + 2] = q.z, w[4 * j + 3] = q.w;
    }
#pragma unroll
    for (int u = 0; u < G::kUnits; ++u) {
      uint32_t raw;
      if constexpr (KIND == CGAN_DTF_SRC_UNITY_D)
        raw = byte_of(w, u * CH) | byte_of(w, u * CH + 1) << 8 | byte_of(w, u * CH + 2) << 16;
      else if constexpr (KIND == CGAN_DTF_SRC_KITTI_D) raw = (w[u >> 1] >> ((u & 1) * 16)) & 0xffffu;
      else if constexpr (KIND == CGAN_DTF_SRC_F32_D) raw = w[u];
      else raw = byte_of(w, u);
      const float v = minmax_value<KIND>(raw, it.far_plane);
      mn = nan_min(mn, v), mx = nan_max(mx, v);
    }
  }
  // the units behind the last whole group: fewer than 16, read one by one by the last part's first thread
  if ((int)blockIdx.x == parts - 1 && threadIdx.x == 0) {
    const uint8_t* b = reinterpret_cast<const uint8_t*>(it.src);
    for (long u = groups * G::kUnits; u < units; ++u) {
      const uint8_t* p = b + u * G::kUnitBytes;
      uint32_t raw = p[0];
      if constexpr (KIND == CGAN_DTF_SRC_UNITY_D) raw |= (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
      else if constexpr (KIND == CGAN_DTF_SRC_KITTI_D) raw |= (uint32_t)p[1] << 8;
      else if constexpr (KIND == CGAN_DTF_SRC_F32_D) raw |= (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
      const float v = minmax_value<KIND>(raw, it.far_plane);
      mn = nan_min(mn, v), mx = nan_max(mx, v);
    }
  }
  block_minmax256(mn, mx, sh);
  if (threadIdx.x == 0) {
    float* o = ws + ((long)blockIdx.y * kParts + blockIdx.x) * 2;
    o[0] = mn, o[1] = mx;
  }
}

template <int KIND, int CH>
__global__ __launch_bounds__(256) void minmax_finish_kernel(const CganDataMinmaxItem* __restrict__ items,
                                                            const float* __restrict__ ws) {
  __shared__ float sh[512];
  const CganDataMinmaxItem it = items[blockIdx.x];
  const int parts = minmax_parts(minmax_units<KIND>(it) / MinmaxGroup<KIND, CH>::kUnits);
  const float* p = ws + ((long)blockIdx.x * kParts + threadIdx.x) * 2;
  const bool have = (int)threadIdx.x < parts;
  float mn = have ? p[0] : __builtin_inff(), mx = have ? p[1] : -__builtin_inff();
  block_minmax256(mn, mx, sh);
  if (threadIdx.x == 0) {
    it.out[0] = mn, it.out[1] = mx - mn;   // t = t - min(t); t = t / max(t): the divisor is max - min in fp32
    it.out[2] = mx, it.out[3] = mx > 127.f ? 1.f : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ bilinear
template <bool U8>
__device__ __forceinline__ float load_px(const void* src, int off, float mn, float rng) {
  if constexpr (U8) return ((float)reinterpret_cast<const uint8_t*>(src)[off] - mn) / rng;   // data.py:386-387
  else return reinterpret_cast<const float*>(src)[off];
}

template <bool U8, int NS, bool NORM>
__global__ __launch_bounds__(256) void data_tf_bilinear_kernel(const CganDataTfItem* __restrict__ items, Affine4 aff) {
  const CganDataTfItem it = items[blockIdx.y];
  const int ohw = it.out_h * it.out_w;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= ohw) return;
  const int oy = p / it.out_w, ox = p - oy * it.out_w;
  const int y = it.map[NS].row_off + oy, x = map_col(it.map[NS], ox);
  float* dst = reinterpret_cast<float*>(it.dst) + p;

  // row and column offsets of the taps in the source, and the weights, from the output pixel down
  constexpr int T = NS == 0 ? 1 : (NS == 1 ? 2 : 4);
  int ro[T], co[T];
  float LY = 0.f, LX = 0.f, ly[2] = {0.f, 0.f}, lx[2] = {0.f, 0.f};
  if constexpr (NS == 0) {
    ro[0] = y * it.stride_h;
    co[0] = x * it.stride_w;
  } else if constexpr (NS == 1) {
    int a0, a1;
    bil_axis(y, it.stage[0].in_h, it.stage[0].out_h, a0, a1, ly[0]);
    ro[0] = (it.map[0].row_off + a0) * it.stride_h;
    ro[1] = (it.map[0].row_off + a1) * it.stride_h;
    bil_axis(x, it.stage[0].in_w, it.stage[0].out_w, a0, a1, lx[0]);
    co[0] = map_col(it.map[0], a0) * it.stride_w;
    co[1] = map_col(it.map[0], a1) * it.stride_w;
  } else {
    int Y[2], X[2];
    bil_axis(y, it.stage[1].in_h, it.stage[1].out_h, Y[0], Y[1], LY);
    bil_axis(x, it.stage[1].in_w, it.stage[1].out_w, X[0], X[1], LX);
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      int a0, a1;
      bil_axis(it.map[1].row_off + Y[a], it.stage[0].in_h, it.stage[0].out_h, a0, a1, ly[a]);
      ro[2 * a] = (it.map[0].row_off + a0) * it.stride_h;
      ro[2 * a + 1] = (it.map[0].row_off + a1) * it.stride_h;
      bil_axis(map_col(it.map[1], X[a]), it.stage[0].in_w, it.stage[0].out_w, a0, a1, lx[a]);
      co[2 * a] = map_col(it.map[0], a0) * it.stride_w;
      co[2 * a + 1] = map_col(it.map[0], a1) * it.stride_w;
    }
  }
  // an x source whose min / max the host has not computed: cgan_data_source_minmax left them earlier on this stream
  const float u8_min = U8 && it.stats ? it.stats[0] : it.u8_min, u8_range = U8 && it.stats ? it.stats[1] : it.u8_range;
  for (int c = 0; c < it.channels; ++c) {
    const int cb = c * it.stride_c;
    float t[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j) t[i][j] = load_px<U8>(it.src, cb + ro[i] + co[j], u8_min, u8_range);
    float v;
    if constexpr (NS == 0) {
      v = t[0][0];
    } else if constexpr (NS == 1) {
      v = bil4(ly[0], lx[0], t[0][0], t[0][1], t[1][0], t[1][1]);
    } else {
      // the four stage-1 pixels the second resampling reads, each a bilinear sample of the source
      float s[2][2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
          s[a][b] = bil4(ly[a], lx[b], t[2 * a][2 * b], t[2 * a][2 * b + 1], t[2 * a + 1][2 * b], t[2 * a + 1][2 * b + 1]);
      v = bil4(LY, LX, s[0][0], s[0][1], s[1][0], s[1][1]);
    }
    if constexpr (NORM) v = (v - aff.mean[c & 3]) / aff.std[c & 3];   // Normalize, transforms.py:214-237
    CGAN_ST_STREAM(v, dst + c * ohw);
  }
}

// ------------------------------------------------------------------------------------------------ colour jitter
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }
__device__ __forceinline__ float blend(float a, float b, float f, float omf) {
  return fminf(fmaxf(f * a + omf * b, 0.f), 1.f);
}

__device__ inline float block_sum256(float v, float* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const float r = sh[0];
  __syncthreads();
  return r;
}

// pass 1 of the contrast item: `parts` fixed-range partial sums of gray per image (the pattern of diffaug.hip)
__global__ __launch_bounds__(256) void jitter_gray_sum_kernel(const float* __restrict__ x, float* __restrict__ ws, int hw,
                                                              int parts) {
  __shared__ float sh[256];
  const float* xi = x + (long)blockIdx.y * 3 * hw;
  const int chunk = (hw + parts - 1) / parts;
  const int lo = blockIdx.x * chunk, hi = lo + chunk < hw ? lo + chunk : hw;
  float s = 0.f;
  for (int k = lo + threadIdx.x; k < hi; k += 256) s += gray_of(xi[k], xi[hw + k], xi[2 * hw + k]);
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) ws[(long)blockIdx.y * kParts + blockIdx.x] = s;
}

template <bool NORM>
__global__ __launch_bounds__(256) void jitter_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                     const float* __restrict__ factors, int op, int hw,
                                                     const float* __restrict__ ws, int parts, Affine4 aff) {
  __shared__ float sh[256];
  const int n = blockIdx.y;
  const float f = factors[2 * n], omf = factors[2 * n + 1];
  float mean = 0.f;
  if (op == CGAN_JIT_CONTRAST)
    mean = block_sum256((int)threadIdx.x < parts ? ws[(long)n * kParts + threadIdx.x] : 0.f, sh) / (float)hw;
  const float* xi = x + (long)n * 3 * hw;
  float* yi = y + (long)n * 3 * hw;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < hw; p += gridDim.x * 256) {
    float v[3] = {CGAN_LD_STREAM(xi + p), CGAN_LD_STREAM(xi + hw + p), CGAN_LD_STREAM(xi + 2 * hw + p)};
    const float other = op == CGAN_JIT_BRIGHTNESS ? 0.f : (op == CGAN_JIT_SATURATION ? gray_of(v[0], v[1], v[2]) : mean);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float o = blend(v[c], other, f, omf);
      // "dummy pixels to fool scaling and preserve range" (transforms.py:504-506): [0, 0] = 1, then [-1, -1] = 0
      if (p == 0) o = 1.f;
      if (p == hw - 1) o = 0.f;
      if constexpr (NORM) o = (o - aff.mean[c]) / aff.std[c];
      CGAN_ST_STREAM(o, yi + c * hw + p);
    }
  }
}

// A run-time choice as a template argument: calls f(std::integral_constant<int, v>) for v in [0, N)
template <int N, typename F>
void static_int(int v, F&& f) {
  if constexpr (N > 0) {
    if (v == N - 1) f(std::integral_constant<int, N - 1>{});
    else static_int<N - 1>(v, f);
  }
}

bool window_inside(const CganDataTfMap& m, int wh, int ww, int H, int W) {
  if (m.row_off < 0 || (long)m.row_off + wh > H) return false;
  if (m.flip) return m.col_off <= W - 1 && (long)m.col_off - (ww - 1) >= 0;
  return m.col_off >= 0 && (long)m.col_off + ww <= W;
}

}  // namespace

extern "C" int cgan_data_transform(const CganDataTfItem* items_host, const CganDataTfItem* items_device, int32_t count,
                                   int32_t mode, int32_t src_kind, int32_t epilogue, const float* mean, const float* std,
                                   const float* boundaries, int32_t n_boundaries, const CganDataTfPalette* palette,
                                   void* stream) {
  CGAN_REQUIRE(items_host && items_device && count > 0 && count <= 65535, "data_transform: bad item table");
  CGAN_REQUIRE(mode == CGAN_DTF_NEAREST || mode == CGAN_DTF_BILINEAR, "data_transform: bad mode %d", mode);
  CGAN_REQUIRE(src_kind >= CGAN_DTF_SRC_B4 && src_kind <= CGAN_DTF_SRC_SEG_NEAREST, "data_transform: bad source kind %d",
               src_kind);
  const bool raw = src_kind >= CGAN_DTF_SRC_UNITY_D;
  const bool raw_depth = src_kind == CGAN_DTF_SRC_UNITY_D || src_kind == CGAN_DTF_SRC_KITTI_D || src_kind == CGAN_DTF_SRC_F32_D;
  const bool seg = src_kind == CGAN_DTF_SRC_SEG_EXACT || src_kind == CGAN_DTF_SRC_SEG_NEAREST;
  CGAN_REQUIRE(epilogue == CGAN_DTF_EPI_NONE || epilogue == CGAN_DTF_EPI_NORMALIZE || epilogue == CGAN_DTF_EPI_BUCKETIZE,
               "data_transform: bad epilogue %d", epilogue);
  if (mode == CGAN_DTF_BILINEAR) {
    CGAN_REQUIRE(src_kind != CGAN_DTF_SRC_B8, "data_transform: bilinear reads fp32 or uint8 sources");
    CGAN_REQUIRE(epilogue != CGAN_DTF_EPI_BUCKETIZE, "data_transform: bucketize belongs to the nearest mode");
    CGAN_REQUIRE(epilogue != CGAN_DTF_EPI_NORMALIZE || (mean && std), "data_transform: normalize needs mean and std");
  } else {
    CGAN_REQUIRE(src_kind != CGAN_DTF_SRC_U8, "data_transform: uint8 sources are read by the bilinear mode only");
    CGAN_REQUIRE(epilogue != CGAN_DTF_EPI_NORMALIZE, "data_transform: normalize belongs to the bilinear mode");
    CGAN_REQUIRE(epilogue != CGAN_DTF_EPI_BUCKETIZE ||
                     ((src_kind == CGAN_DTF_SRC_B4 || raw_depth) && boundaries && n_boundaries > 0),
                 "data_transform: bucketize needs fp32 or raw depth sources and a boundaries array");
  }
  CGAN_REQUIRE(!raw || mode == CGAN_DTF_NEAREST, "data_transform: raw sources are read by the nearest mode only");
  CGAN_REQUIRE(seg == (palette != nullptr), "data_transform: a palette goes with the segmentation kinds, and only with them");
  CganDataTfPalette pal = {};
  if (seg) {
    pal = *palette;
    CGAN_REQUIRE(pal.n >= 1 && pal.n <= 16, "data_transform: a palette holds 1 to 16 colours, got %d", pal.n);
    for (int i = 0; i < pal.n; ++i)
      CGAN_REQUIRE(src_kind != CGAN_DTF_SRC_SEG_EXACT || (pal.colour[i] >> 24) == 0,
                   "data_transform: palette colour %d of a 3-channel source has an alpha byte", i);
  }
  const int ns = items_host[0].n_stages;
  CGAN_REQUIRE(ns >= 0 && ns <= 2, "data_transform: a plan has 0 to 2 resampling stages, got %d", ns);
  long max_pix = 0;
  for (int k = 0; k < count; ++k) {
    const CganDataTfItem& it = items_host[k];
    CGAN_REQUIRE(it.src && it.dst, "data_transform: item %d: null pointer", k);
    CGAN_REQUIRE(it.n_stages == ns, "data_transform: item %d has %d stages, item 0 has %d", k, it.n_stages, ns);
    CGAN_REQUIRE(it.src_h > 0 && it.src_w > 0 && it.channels > 0 && it.out_h > 0 && it.out_w > 0,
                 "data_transform: item %d: bad shape", k);
    CGAN_REQUIRE(epilogue != CGAN_DTF_EPI_NORMALIZE || it.channels <= 4, "data_transform: normalize takes at most 4 channels");
    CGAN_REQUIRE(it.stride_c >= 0 && it.stride_h >= 0 && it.stride_w >= 0 &&
                     (long)(it.channels - 1) * it.stride_c + (long)(it.src_h - 1) * it.stride_h +
                             (long)(it.src_w - 1) * it.stride_w < (1l << 31),
                 "data_transform: item %d: source strides outside 32-bit offsets", k);
    CGAN_REQUIRE((long)it.channels * it.out_h * it.out_w < (1l << 31), "data_transform: item %d: output too large", k);
    CGAN_REQUIRE(src_kind != CGAN_DTF_SRC_U8 || it.stats || it.u8_range != 0.f, "data_transform: item %d: zero uint8 range", k);
    CGAN_REQUIRE(raw || src_kind == CGAN_DTF_SRC_U8 || !it.stats, "data_transform: item %d: stats go with uint8 and raw sources", k);
    if (raw) {
      // the element size is the kind's: the channel count and the strides say what the kernel will read
      const bool chans = src_kind == CGAN_DTF_SRC_UNITY_D ? (it.channels == 3 || it.channels == 4)
                         : src_kind == CGAN_DTF_SRC_SEG_EXACT ? it.channels == 3
                         : src_kind == CGAN_DTF_SRC_SEG_NEAREST ? it.channels == 4
                         : src_kind == CGAN_DTF_SRC_MASK ? it.channels >= 1 : it.channels == 1;
      CGAN_REQUIRE(chans, "data_transform: item %d: %d channels do not fit source kind %d", k, it.channels, src_kind);
      const int known = raw_depth ? (CGAN_DTF_DEC_LOG | CGAN_DTF_DEC_NORMALIZE) : (src_kind == CGAN_DTF_SRC_MASK ? CGAN_DTF_DEC_THRESHOLD : 0);
      CGAN_REQUIRE((it.dec_flags & ~known) == 0, "data_transform: item %d: decode flags %d do not fit source kind %d", k,
                   it.dec_flags, src_kind);
      CGAN_REQUIRE(!((it.dec_flags & CGAN_DTF_DEC_LOG) && (it.dec_flags & CGAN_DTF_DEC_NORMALIZE)),
                   "data_transform: item %d: normalize and log exclude each other", k);
      CGAN_REQUIRE(src_kind != CGAN_DTF_SRC_F32_D || !(it.dec_flags & CGAN_DTF_DEC_LOG),
                   "data_transform: item %d: the fp32 depth is normalised, never log", k);
      const bool divides = src_kind == CGAN_DTF_SRC_F32_D || (it.dec_flags & CGAN_DTF_DEC_NORMALIZE);
      CGAN_REQUIRE(!divides || it.stats || it.u8_range != 0.f, "data_transform: item %d: zero range", k);
      CGAN_REQUIRE(src_kind != CGAN_DTF_SRC_UNITY_D || it.far_plane > 0.f, "data_transform: item %d: far plane %g", k,
                   (double)it.far_plane);
      CGAN_REQUIRE(src_kind != CGAN_DTF_SRC_KITTI_D || ((uintptr_t)it.src & 1) == 0, "data_transform: item %d: unaligned uint16 source", k);
      CGAN_REQUIRE(src_kind != CGAN_DTF_SRC_F32_D || ((uintptr_t)it.src & 3) == 0, "data_transform: item %d: unaligned fp32 source", k);
    }
    // every window inside the image below it: the sampled indices are clamped to the window, so nothing leaves the source
    int wh = it.out_h, ww = it.out_w;
    for (int s = ns; s >= 0; --s) {
      int H = it.src_h, W = it.src_w;
      if (s > 0) {
        const CganDataTfStage& st = it.stage[s - 1];
        CGAN_REQUIRE(st.in_h > 0 && st.in_w > 0 && st.out_h > 0 && st.out_w > 0, "data_transform: item %d: bad stage", k);
        H = st.out_h, W = st.out_w;
      }
      CGAN_REQUIRE(window_inside(it.map[s], wh, ww, H, W),
                   "data_transform: item %d: window %d x %d of map %d leaves its %d x %d image", k, wh, ww, s, H, W);
      if (s > 0) wh = it.stage[s - 1].in_h, ww = it.stage[s - 1].in_w;
    }
    const long pix = (long)it.out_h * it.out_w;
    max_pix = pix > max_pix ? pix : max_pix;
  }
  Affine4 aff = {{0.f, 0.f, 0.f, 0.f}, {1.f, 1.f, 1.f, 1.f}};
  if (epilogue == CGAN_DTF_EPI_NORMALIZE)
    for (int c = 0; c < 4; ++c) {
      CGAN_REQUIRE(std[c] != 0.f, "data_transform: std[%d] is zero", c);
      aff.mean[c] = mean[c], aff.std[c] = std[c];
    }
  hipStream_t s = (hipStream_t)stream;
  if (mode == CGAN_DTF_NEAREST) {
    const dim3 grid((unsigned)((max_pix + 256 * kNearPix - 1) / (256 * kNearPix)), count);
    static_int<CGAN_DTF_SRC_SEG_NEAREST + 1>(src_kind, [&](auto K) {
      static_int<3>(ns, [&](auto NS) {
        static_int<2>(epilogue == CGAN_DTF_EPI_BUCKETIZE, [&](auto B) {
          constexpr int kind = decltype(K)::value;
          constexpr bool bucket = decltype(B)::value;
          // uint8 is the bilinear mode's; only fp32 values bucketize: the 4-byte gather and the raw depths (checked above)
          constexpr bool depth = kind == CGAN_DTF_SRC_UNITY_D || kind == CGAN_DTF_SRC_KITTI_D || kind == CGAN_DTF_SRC_F32_D;
          if constexpr (kind != CGAN_DTF_SRC_U8 && (!bucket || kind == CGAN_DTF_SRC_B4 || depth))
            hipLaunchKernelGGL((data_tf_nearest_kernel<kind, decltype(NS)::value, bucket>), grid, dim3(256), 0, s, items_device,
                               boundaries, n_boundaries, pal);
        });
      });
    });
  } else {
    const dim3 grid((unsigned)((max_pix + 255) / 256), count);
    static_int<2>(src_kind == CGAN_DTF_SRC_U8, [&](auto U) {
      static_int<3>(ns, [&](auto NS) {
        static_int<2>(epilogue == CGAN_DTF_EPI_NORMALIZE, [&](auto N) {
          hipLaunchKernelGGL((data_tf_bilinear_kernel<decltype(U)::value != 0, decltype(NS)::value, decltype(N)::value != 0>),
                             grid, dim3(256), 0, s, items_device, aff);
        });
      });
    });
  }
  CGAN_CHECK_LAUNCH("data_transform");
  return CGAN_OK;
}

extern "C" int cgan_data_source_minmax(const CganDataMinmaxItem* items_host, const CganDataMinmaxItem* items_device,
                                       int32_t count, int32_t src_kind, float* ws, void* stream) {
  CGAN_REQUIRE(items_host && items_device && ws && count > 0 && count <= 65535, "data_source_minmax: bad item table");
  CGAN_REQUIRE(src_kind == CGAN_DTF_SRC_U8 || src_kind == CGAN_DTF_SRC_MASK || src_kind == CGAN_DTF_SRC_UNITY_D ||
                   src_kind == CGAN_DTF_SRC_KITTI_D || src_kind == CGAN_DTF_SRC_F32_D,
               "data_source_minmax: bad source kind %d", src_kind);
  const int ch = items_host[0].channels;
  for (int k = 0; k < count; ++k) {
    const CganDataMinmaxItem& it = items_host[k];
    CGAN_REQUIRE(it.src && it.out, "data_source_minmax: item %d: null pointer", k);
    CGAN_REQUIRE(((uintptr_t)it.src & 15) == 0, "data_source_minmax: item %d: the source is not 16-byte aligned", k);
    CGAN_REQUIRE(it.pixels > 0 && it.channels > 0 && it.pixels < (1l << 40) / it.channels, "data_source_minmax: item %d: bad size", k);
    if (src_kind == CGAN_DTF_SRC_UNITY_D) {
      CGAN_REQUIRE(it.channels == 3 || it.channels == 4, "data_source_minmax: item %d: a Unity depth code has 3 or 4 channels", k);
      CGAN_REQUIRE(it.channels == ch, "data_source_minmax: item %d has %d channels, item 0 has %d", k, it.channels, ch);
      CGAN_REQUIRE(it.far_plane > 0.f, "data_source_minmax: item %d: far plane %g", k, (double)it.far_plane);
    } else if (src_kind == CGAN_DTF_SRC_KITTI_D || src_kind == CGAN_DTF_SRC_F32_D) {
      CGAN_REQUIRE(it.channels == 1, "data_source_minmax: item %d: a depth map has one channel", k);
    }
  }
  hipStream_t s = (hipStream_t)stream;
#define MINMAX(K, CH) \
  do { \
    hipLaunchKernelGGL((minmax_partial_kernel<K, CH>), dim3(kParts, count), dim3(256), 0, s, items_device, ws); \
    CGAN_CHECK_LAUNCH("data_source_minmax_partial"); \
    hipLaunchKernelGGL((minmax_finish_kernel<K, CH>), dim3(count), dim3(256), 0, s, items_device, (const float*)ws); \
  } while (0)
  if (src_kind == CGAN_DTF_SRC_UNITY_D) {
    if (ch == 3) MINMAX(CGAN_DTF_SRC_UNITY_D, 3); else MINMAX(CGAN_DTF_SRC_UNITY_D, 4);
  } else if (src_kind == CGAN_DTF_SRC_KITTI_D) MINMAX(CGAN_DTF_SRC_KITTI_D, 1);
  else if (src_kind == CGAN_DTF_SRC_F32_D) MINMAX(CGAN_DTF_SRC_F32_D, 1);
  else MINMAX(CGAN_DTF_SRC_U8, 1);
#undef MINMAX
  CGAN_CHECK_LAUNCH("data_source_minmax_finish");
  return CGAN_OK;
}

extern "C" int cgan_data_jitter(const float* x, float* y, const float* factors, int32_t op, int32_t n, int32_t h, int32_t w,
                                const float* mean, const float* std, float* ws, void* stream) {
  CGAN_REQUIRE(x && y && factors && x != y, "data_jitter: null or aliased pointer");
  CGAN_REQUIRE(op == CGAN_JIT_BRIGHTNESS || op == CGAN_JIT_SATURATION || op == CGAN_JIT_CONTRAST, "data_jitter: bad op %d", op);
  CGAN_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0 && (long)h * w * 3 < (1l << 31), "data_jitter: bad shape");
  CGAN_REQUIRE(op != CGAN_JIT_CONTRAST || ws, "data_jitter: contrast needs a workspace");
  CGAN_REQUIRE((mean == nullptr) == (std == nullptr), "data_jitter: mean and std come together");
  const int hw = h * w;
  long p = ((long)hw + 4095) / 4096;
  const int parts = (int)(p < 1 ? 1 : (p > kParts ? kParts : p));
  hipStream_t s = (hipStream_t)stream;
  if (op == CGAN_JIT_CONTRAST) {
    hipLaunchKernelGGL(jitter_gray_sum_kernel, dim3(parts, n), dim3(256), 0, s, x, ws, hw, parts);
    CGAN_CHECK_LAUNCH("data_jitter_sum");
  }
  long blocks = ((long)hw + 255) / 256, cap = 16384 / n;
  if (cap < 4) cap = 4;
  const dim3 grid((unsigned)(blocks < cap ? blocks : cap), n);
  Affine4 aff = {{0.f, 0.f, 0.f, 0.f}, {1.f, 1.f, 1.f, 1.f}};
  if (mean) {
    for (int c = 0; c < 3; ++c) {
      CGAN_REQUIRE(std[c] != 0.f, "data_jitter: std[%d] is zero", c);
      aff.mean[c] = mean[c], aff.std[c] = std[c];
    }
    hipLaunchKernelGGL(jitter_kernel<true>, grid, dim3(256), 0, s, x, y, factors, op, hw, (const float*)ws, parts, aff);
  } else {
    hipLaunchKernelGGL(jitter_kernel<false>, grid, dim3(256), 0, s, x, y, factors, op, hw, (const float*)ws, parts, aff);
  }
  CGAN_CHECK_LAUNCH("data_jitter");
  return CGAN_OK;
}
