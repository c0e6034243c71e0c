// Differentiable augmentation of the Painter's discriminator inputs (DiffAugment: reference climategan/transforms.py:494-626,
// applied by trainer.py:1079-1081 and :1319-1321): per image, brightness -> contrast -> saturation, then translation with
// zero fill, then a cutout box.  Two forms, each a forward and a backward:
//   cgan_diffaug_fwd / _bwd                      NCHW fp32 -> NCHW fp32 (the public transform, the local / global pair)
//   cgan_painter_heads_diffaug_fwd / _bwd        fused into the Painter heads: the paste, the augmentation, [m | p_aug]
//                                                as the 16-bit discriminator input and vgg_preprocess of the UN-augmented p
// The contrast mean is the only cross-pixel quantity: pass 1 writes CGAN_DIFFAUG_PARTS fixed-range partial sums per image,
// pass 2 sums them in a fixed tree before its per-pixel gather.  No atomics: results are run-to-run identical.
#include "cgan_common.h"

namespace {

constexpr int kParts = CGAN_DIFFAUG_PARTS;

// one image's parameters, derived from the raw draws with the reference's own fp32 expressions
struct Aug {
  bool bright, contrast, sat;
  float b, cf, sf;       // rand - 0.5 (:501), rand + 0.5 (:534), rand * 2 (:518)
  int tx, ty;            // out[i][j] = in[i + tx][j + ty], 0 outside (:580-606)
  int r0, r1, c0, c1;    // cutout rows [r0, r1] x cols [c0, c1] (:544-577); r1 < r0: no box
};

__device__ inline int clampi(long v, int lo, int hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }

__device__ inline Aug load_aug(const float* color, const int64_t* geo, int flags, int cut_h, int cut_w, int n, int h,
                               int w) {
  Aug a;
  a.bright = (flags & CGAN_DA_BRIGHTNESS) != 0;
  a.contrast = (flags & CGAN_DA_CONTRAST) != 0;
  a.sat = (flags & CGAN_DA_SATURATION) != 0;
  a.b = a.bright ? color[n * 3 + 0] - 0.5f : 0.f;
  a.cf = a.contrast ? color[n * 3 + 1] + 0.5f : 1.f;
  a.sf = a.sat ? color[n * 3 + 2] * 2.f : 1.f;
  const bool tr = (flags & CGAN_DA_TRANSLATION) != 0;
  a.tx = tr ? (int)geo[n * 4 + 0] : 0;
  a.ty = tr ? (int)geo[n * 4 + 1] : 0;
  a.r0 = 0, a.r1 = -1, a.c0 = 0, a.c1 = -1;
  if ((flags & CGAN_DA_CUTOUT) && cut_h > 0 && cut_w > 0) {
    // the zeroed rows are clamp(k + ox - cut_h / 2, 0, h - 1) for k in [0, cut_h): clamp is monotone, so that set is the
    // contiguous range between the clamped ends (the same for the columns; the box is their product)
    const long r = geo[n * 4 + 2] - cut_h / 2, c = geo[n * 4 + 3] - cut_w / 2;
    a.r0 = clampi(r, 0, h - 1), a.r1 = clampi(r + cut_h - 1, 0, h - 1);
    a.c0 = clampi(c, 0, w - 1), a.c1 = clampi(c + cut_w - 1, 0, w - 1);
  }
  return a;
}

__device__ inline bool is_cut(const Aug& a, int i, int j) { return i >= a.r0 && i <= a.r1 && j >= a.c0 && j <= a.c1; }

// output pixel (i, j) shows input pixel (i + tx, j + ty) unless that lies outside the image or (i, j) is cut out
__device__ inline bool visible(const Aug& a, int i, int j, int h, int w) {
  const int si = i + a.tx, sj = j + a.ty;
  return si >= 0 && si < h && sj >= 0 && sj < w && !is_cut(a, i, j);
}

// brightness then contrast of one value; mean = the brightened image's mean
__device__ inline float bc(const Aug& a, float v, float mean) {
  if (a.bright) v = v + a.b;
  if (a.contrast) v = (v - mean) * a.cf + mean;
  return v;
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

// this image's total from pass 1's partials (fixed order)
__device__ inline float image_total(const float* ws, int n, int parts, float* sh) {
  return block_sum256((int)threadIdx.x < parts ? ws[(long)n * kParts + threadIdx.x] : 0.f, sh);
}

// block (b, n) of pass 1 covers [b * chunk, (b + 1) * chunk) of image n's len items
__device__ inline void part_range(long len, int parts, long& lo, long& hi) {
  const long chunk = (len + parts - 1) / parts;
  lo = (long)blockIdx.x * chunk;
  hi = lo + chunk < len ? lo + chunk : len;
}

// ------------------------------------------------------------------------------------------------ NCHW fp32
__global__ __launch_bounds__(256) void diffaug_sum_kernel(const float* __restrict__ x, float* __restrict__ ws, long len,
                                                          int parts) {
  __shared__ float sh[256];
  const int n = blockIdx.y;
  long lo, hi;
  part_range(len, parts, lo, hi);
  float s = 0.f;
  for (long k = lo + threadIdx.x; k < hi; k += 256) s += x[(long)n * len + k];
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) ws[(long)n * kParts + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void diffaug_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                          const float* __restrict__ color, const int64_t* __restrict__ geo,
                                                          int flags, int cut_h, int cut_w, int c, int h, int w,
                                                          const float* __restrict__ ws, int parts) {
  __shared__ float sh[256];
  const int n = blockIdx.y;
  const Aug a = load_aug(color, geo, flags, cut_h, cut_w, n, h, w);
  const long hw = (long)h * w;
  const float mean = a.contrast ? image_total(ws, n, parts, sh) / (float)(c * hw) + a.b : 0.f;
  const float* xi = x + (long)n * c * hw;
  float* yi = y + (long)n * c * hw;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < hw; p += (long)gridDim.x * 256) {
    const int i = (int)(p / w), j = (int)(p - (long)i * w);
    if (!visible(a, i, j, h, w)) {
      for (int k = 0; k < c; ++k) yi[k * hw + p] = 0.f;
      continue;
    }
    const long q = (long)(i + a.tx) * w + (j + a.ty);
    float mc = 0.f;
    if (a.sat) {
      for (int k = 0; k < c; ++k) mc += bc(a, xi[k * hw + q], mean);
      mc = mc / (float)c;
    }
    for (int k = 0; k < c; ++k) {
      const float v = bc(a, xi[k * hw + q], mean);
      yi[k * hw + p] = a.sat ? (v - mc) * a.sf + mc : v;
    }
  }
}

// sum over the visible output pixels of dy (= the sum of the gradient reaching the contrast step)
__global__ __launch_bounds__(256) void diffaug_bwd_sum_kernel(const float* __restrict__ dy, const float* __restrict__ color,
                                                              const int64_t* __restrict__ geo, int flags, int cut_h,
                                                              int cut_w, int c, int h, int w, float* __restrict__ ws,
                                                              int parts) {
  __shared__ float sh[256];
  const int n = blockIdx.y;
  const Aug a = load_aug(color, geo, flags, cut_h, cut_w, n, h, w);
  const long hw = (long)h * w;
  long lo, hi;
  part_range(hw, parts, lo, hi);
  float s = 0.f;
  for (long p = lo + threadIdx.x; p < hi; p += 256) {
    const int i = (int)(p / w), j = (int)(p - (long)i * w);
    if (visible(a, i, j, h, w))
      for (int k = 0; k < c; ++k) s += dy[((long)n * c + k) * hw + p];
  }
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) ws[(long)n * kParts + blockIdx.x] = s;
}

// input pixel q receives output pixel q - t's gradient (gather: the translation is one-to-one), then
// saturation backward sf g + (1 - sf) mean_c(g), contrast backward cf g + (1 - cf) sum(g) / (c h w); brightness: identity
__global__ __launch_bounds__(256) void diffaug_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx,
                                                          const float* __restrict__ color, const int64_t* __restrict__ geo,
                                                          int flags, int cut_h, int cut_w, int c, int h, int w,
                                                          const float* __restrict__ ws, int parts) {
  __shared__ float sh[256];
  const int n = blockIdx.y;
  const Aug a = load_aug(color, geo, flags, cut_h, cut_w, n, h, w);
  const long hw = (long)h * w;
  const float gmean = a.contrast ? image_total(ws, n, parts, sh) / (float)(c * hw) : 0.f;
  const float* dyi = dy + (long)n * c * hw;
  float* dxi = dx + (long)n * c * hw;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < hw; q += (long)gridDim.x * 256) {
    const int si = (int)(q / w), sj = (int)(q - (long)si * w);
    const int i = si - a.tx, j = sj - a.ty;
    const bool vis = i >= 0 && i < h && j >= 0 && j < w && !is_cut(a, i, j);
    const long p = (long)i * w + j;
    float mg = 0.f;
    if (a.sat && vis) {
      for (int k = 0; k < c; ++k) mg += dyi[k * hw + p];
      mg = mg / (float)c;
    }
    for (int k = 0; k < c; ++k) {
      float g = vis ? dyi[k * hw + p] : 0.f;
      if (a.sat) g = a.sf * g + (1.f - a.sf) * mg;
      if (a.contrast) g = a.cf * g + (1.f - a.cf) * gmean;
      dxi[k * hw + q] = g;
    }
  }
}

// ------------------------------------------------------------------------------------------------ fused Painter heads
// p = fake ? x (1 - m) + fake m : x at pixel idx of image n (the paste of painter_heads_fwd_kernel, same expression)
template <typename T>
__device__ inline void paste3(const uint16_t* fake, const float* x, const float* m, long n, long hw, long pix, float pc[3]) {
  const long idx = n * hw + pix;
  const float mv = m[idx];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float xv = x[(n * 3 + c) * hw + pix];
    pc[c] = fake ? xv * (1.f - mv) + f32_of_bits<T>(fake[idx * 8 + c]) * mv : xv;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void heads_diffaug_sum_kernel(const uint16_t* __restrict__ fake, const float* __restrict__ x,
                                                                const float* __restrict__ m, float* __restrict__ ws, long hw,
                                                                int parts) {
  __shared__ float sh[256];
  const int n = blockIdx.y;
  long lo, hi;
  part_range(hw, parts, lo, hi);
  float s = 0.f;
  for (long p = lo + threadIdx.x; p < hi; p += 256) {
    float pc[3];
    paste3<T>(fake, x, m, n, hw, p, pc);
    s += pc[0] + pc[1] + pc[2];
  }
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) ws[(long)n * kParts + blockIdx.x] = s;
}

// d_in = [m | augment(p)] (the mask channel is neither jittered nor moved, trainer.py:1101-1102 / :1360-1361);
// vgg_in = vgg_preprocess(p * m) of the un-augmented p, bit for bit painter_heads_fwd_kernel's
template <typename T>
__global__ __launch_bounds__(256) void heads_diffaug_fwd_kernel(const uint16_t* __restrict__ fake, const float* __restrict__ x,
                                                                const float* __restrict__ m, uint16_t* __restrict__ d_in,
                                                                uint16_t* __restrict__ vgg_in, const float* __restrict__ color,
                                                                const int64_t* __restrict__ geo, int flags, int cut_h,
                                                                int cut_w, int h, int w, const float* __restrict__ ws,
                                                                int parts) {
  __shared__ float sh[256];
  const int n = blockIdx.y;
  const Aug a = load_aug(color, geo, flags, cut_h, cut_w, n, h, w);
  const long hw = (long)h * w;
  const float mean = a.contrast ? image_total(ws, n, parts, sh) / (float)(3 * hw) + a.b : 0.f;
  for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < hw; p += (long)gridDim.x * 256) {
    const long i_out = (long)n * hw + p;
    const int i = (int)(p / w), j = (int)(p - (long)i * w);
    const float mv = m[i_out];
    float o[3] = {0.f, 0.f, 0.f};
    if (visible(a, i, j, h, w)) {
      float pc[3];
      paste3<T>(fake, x, m, n, hw, (long)(i + a.tx) * w + (j + a.ty), pc);
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = bc(a, pc[c], mean);
      if (a.sat) {
        const float mc = (o[0] + o[1] + o[2]) / 3.f;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = (o[c] - mc) * a.sf + mc;
      }
    }
    u32x4 d;
    d[0] = pack2<T>(mv, o[0]);
    d[1] = pack2<T>(o[1], o[2]);
    d[2] = 0u;
    d[3] = 0u;
    reinterpret_cast<u32x4*>(d_in)[i_out] = d;
    if (vgg_in) {
      float pc[3];
      paste3<T>(fake, x, m, n, hw, p, pc);
      const float b = (pc[2] * mv + 1.f) * 255.f * 0.5f - 103.939f;
      const float g = (pc[1] * mv + 1.f) * 255.f * 0.5f - 116.779f;
      const float r = (pc[0] * mv + 1.f) * 255.f * 0.5f - 123.680f;
      const float bh = f32_of_bits<T>(bits_of<T>(b)), gh = f32_of_bits<T>(bits_of<T>(g)), rh = f32_of_bits<T>(bits_of<T>(r));
      u32x4 v;
      v[0] = pack2<T>(bh, gh);
      v[1] = pack2<T>(rh, b - bh);
      v[2] = pack2<T>(g - gh, r - rh);
      v[3] = 0u;
      reinterpret_cast<u32x4*>(vgg_in)[i_out] = v;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void heads_diffaug_bwd_sum_kernel(const uint16_t* __restrict__ dd,
                                                                    const float* __restrict__ color,
                                                                    const int64_t* __restrict__ geo, int flags, int cut_h,
                                                                    int cut_w, int h, int w, float* __restrict__ ws,
                                                                    int parts) {
  __shared__ float sh[256];
  const int n = blockIdx.y;
  const Aug a = load_aug(color, geo, flags, cut_h, cut_w, n, h, w);
  const long hw = (long)h * w;
  long lo, hi;
  part_range(hw, parts, lo, hi);
  float s = 0.f;
  for (long p = lo + threadIdx.x; p < hi; p += 256) {
    const int i = (int)(p / w), j = (int)(p - (long)i * w);
    if (visible(a, i, j, h, w)) {
      const long o = ((long)n * hw + p) * 8;
      s += f32_of_bits<T>(dd[o + 1]) + f32_of_bits<T>(dd[o + 2]) + f32_of_bits<T>(dd[o + 3]);
    }
  }
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) ws[(long)n * kParts + blockIdx.x] = s;
}

// d_fake[c] = m * (augment_bwd(d_d_in[1..3])[c] + 127.5 m d_vgg_in[2 - c])     (painter_heads_bwd_kernel with the
// augmentation's backward in front of the discriminator half)
template <typename T>
__global__ __launch_bounds__(256) void heads_diffaug_bwd_kernel(const uint16_t* __restrict__ dd, const uint16_t* __restrict__ dv,
                                                                const float* __restrict__ m, uint16_t* __restrict__ dfake,
                                                                const float* __restrict__ color,
                                                                const int64_t* __restrict__ geo, int flags, int cut_h,
                                                                int cut_w, int h, int w, const float* __restrict__ ws,
                                                                int parts) {
  __shared__ float sh[256];
  const int n = blockIdx.y;
  const Aug a = load_aug(color, geo, flags, cut_h, cut_w, n, h, w);
  const long hw = (long)h * w;
  const float gmean = a.contrast ? image_total(ws, n, parts, sh) / (float)(3 * hw) : 0.f;
  for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < hw; q += (long)gridDim.x * 256) {
    const long i_in = (long)n * hw + q;
    const int si = (int)(q / w), sj = (int)(q - (long)si * w);
    const int i = si - a.tx, j = sj - a.ty;
    float g[3] = {0.f, 0.f, 0.f};
    if (i >= 0 && i < h && j >= 0 && j < w && !is_cut(a, i, j)) {
      const long o = ((long)n * hw + (long)i * w + j) * 8;
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] = f32_of_bits<T>(dd[o + 1 + c]);
    }
    if (a.sat) {
      const float mg = (g[0] + g[1] + g[2]) / 3.f;
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] = a.sf * g[c] + (1.f - a.sf) * mg;
    }
    if (a.contrast) {
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] = a.cf * g[c] + (1.f - a.cf) * gmean;
    }
    const float mv = m[i_in];
    if (dv) {
#pragma unroll
      for (int c = 0; c < 3; ++c) g[c] += 127.5f * mv * f32_of_bits<T>(dv[i_in * 8 + 2 - c]);
    }
    u32x4 o;
    o[0] = pack2<T>(g[0] * mv, g[1] * mv);
    o[1] = pack2<T>(g[2] * mv, 0.f);
    o[2] = 0u;
    o[3] = 0u;
    reinterpret_cast<u32x4*>(dfake)[i_in] = o;
  }
}

// pass 1: parts per image (<= kParts, ~4096 items each); pass 2: blocks per image, ~16 k blocks in all
int parts_for(long len) {
  long p = (len + 4095) / 4096;
  return (int)(p < 1 ? 1 : (p > kParts ? kParts : p));
}
int blocks_for(long hw, int n) {
  long b = (hw + 255) / 256, cap = 16384 / n;
  if (cap < 4) cap = 4;
  return (int)(b < cap ? b : cap);
}

}  // namespace

#define DISPATCH_DA(dtype, KERNEL, ...)                                     \
  do {                                                                      \
    if ((dtype) == CGAN_F16) hipLaunchKernelGGL(KERNEL<F16>, __VA_ARGS__);  \
    else hipLaunchKernelGGL(KERNEL<BF16>, __VA_ARGS__);                     \
  } while (0)

#define DA_CHECK_ARGS(what)                                                                                         \
  CGAN_REQUIRE(color && geo && ws, what ": null pointer");                                                          \
  CGAN_REQUIRE((flags & ~CGAN_DA_ALL) == 0, what ": bad flags %d", flags);                                          \
  CGAN_REQUIRE(cut_h >= 0 && cut_w >= 0, what ": bad cutout size %d x %d", cut_h, cut_w);                          \
  CGAN_REQUIRE(n > 0 && n <= 65535 && h > 0 && w > 0, what ": bad shape")

extern "C" int cgan_diffaug_fwd(const float* x, float* y, const float* color, const int64_t* geo, int32_t flags,
                                int32_t cut_h, int32_t cut_w, int32_t n, int32_t c, int32_t h, int32_t w, float* ws,
                                void* stream) {
  CGAN_REQUIRE(x && y && x != y, "diffaug_fwd: null or aliased pointer");
  DA_CHECK_ARGS("diffaug_fwd");
  CGAN_REQUIRE(c > 0, "diffaug_fwd: bad channel count");
  const long hw = (long)h * w, len = (long)c * hw;
  const int parts = parts_for(len);
  if (flags & CGAN_DA_CONTRAST) {
    hipLaunchKernelGGL(diffaug_sum_kernel, dim3(parts, n), dim3(256), 0, (hipStream_t)stream, x, ws, len, parts);
    CGAN_CHECK_LAUNCH("diffaug_sum");
  }
  hipLaunchKernelGGL(diffaug_fwd_kernel, dim3(blocks_for(hw, n), n), dim3(256), 0, (hipStream_t)stream, x, y, color, geo,
                     flags, cut_h, cut_w, c, h, w, (const float*)ws, parts);
  CGAN_CHECK_LAUNCH("diffaug_fwd");
  return CGAN_OK;
}

extern "C" int cgan_diffaug_bwd(const float* dy, float* dx, const float* color, const int64_t* geo, int32_t flags,
                                int32_t cut_h, int32_t cut_w, int32_t n, int32_t c, int32_t h, int32_t w, float* ws,
                                void* stream) {
  CGAN_REQUIRE(dy && dx && dy != dx, "diffaug_bwd: null or aliased pointer");
  DA_CHECK_ARGS("diffaug_bwd");
  CGAN_REQUIRE(c > 0, "diffaug_bwd: bad channel count");
  const long hw = (long)h * w;
  const int parts = parts_for(hw);
  if (flags & CGAN_DA_CONTRAST) {
    hipLaunchKernelGGL(diffaug_bwd_sum_kernel, dim3(parts, n), dim3(256), 0, (hipStream_t)stream, dy, color, geo, flags,
                       cut_h, cut_w, c, h, w, ws, parts);
    CGAN_CHECK_LAUNCH("diffaug_bwd_sum");
  }
  hipLaunchKernelGGL(diffaug_bwd_kernel, dim3(blocks_for(hw, n), n), dim3(256), 0, (hipStream_t)stream, dy, dx, color, geo,
                     flags, cut_h, cut_w, c, h, w, (const float*)ws, parts);
  CGAN_CHECK_LAUNCH("diffaug_bwd");
  return CGAN_OK;
}

extern "C" int cgan_painter_heads_diffaug_fwd(const void* fake_nhwc, const float* x_nchw, const float* m_nchw, void* d_in,
                                              void* vgg_in, const float* color, const int64_t* geo, int32_t flags,
                                              int32_t cut_h, int32_t cut_w, int32_t dtype, int32_t n, int32_t h, int32_t w,
                                              float* ws, void* stream) {
  CGAN_REQUIRE(x_nchw && m_nchw && d_in, "painter_heads_diffaug_fwd: null pointer");
  CGAN_REQUIRE(dtype == CGAN_F16 || dtype == CGAN_BF16, "painter_heads_diffaug_fwd: bad dtype %d", dtype);
  DA_CHECK_ARGS("painter_heads_diffaug_fwd");
  const long hw = (long)h * w;
  const int parts = parts_for(hw);
  if (flags & CGAN_DA_CONTRAST) {
    DISPATCH_DA(dtype, heads_diffaug_sum_kernel, dim3(parts, n), dim3(256), 0, (hipStream_t)stream,
                (const uint16_t*)fake_nhwc, x_nchw, m_nchw, ws, hw, parts);
    CGAN_CHECK_LAUNCH("painter_heads_diffaug_sum");
  }
  DISPATCH_DA(dtype, heads_diffaug_fwd_kernel, dim3(blocks_for(hw, n), n), dim3(256), 0, (hipStream_t)stream,
              (const uint16_t*)fake_nhwc, x_nchw, m_nchw, (uint16_t*)d_in, (uint16_t*)vgg_in, color, geo, flags, cut_h,
              cut_w, h, w, (const float*)ws, parts);
  CGAN_CHECK_LAUNCH("painter_heads_diffaug_fwd");
  return CGAN_OK;
}

extern "C" int cgan_painter_heads_diffaug_bwd(const void* d_d_in, const void* d_vgg_in, const float* m_nchw, void* d_fake,
                                              const float* color, const int64_t* geo, int32_t flags, int32_t cut_h,
                                              int32_t cut_w, int32_t dtype, int32_t n, int32_t h, int32_t w, float* ws,
                                              void* stream) {
  CGAN_REQUIRE(d_d_in && m_nchw && d_fake, "painter_heads_diffaug_bwd: null pointer");
  CGAN_REQUIRE(dtype == CGAN_F16 || dtype == CGAN_BF16, "painter_heads_diffaug_bwd: bad dtype %d", dtype);
  DA_CHECK_ARGS("painter_heads_diffaug_bwd");
  const long hw = (long)h * w;
  const int parts = parts_for(hw);
  if (flags & CGAN_DA_CONTRAST) {
    DISPATCH_DA(dtype, heads_diffaug_bwd_sum_kernel, dim3(parts, n), dim3(256), 0, (hipStream_t)stream,
                (const uint16_t*)d_d_in, color, geo, flags, cut_h, cut_w, h, w, ws, parts);
    CGAN_CHECK_LAUNCH("painter_heads_diffaug_bwd_sum");
  }
  DISPATCH_DA(dtype, heads_diffaug_bwd_kernel, dim3(blocks_for(hw, n), n), dim3(256), 0, (hipStream_t)stream,
              (const uint16_t*)d_d_in, (const uint16_t*)d_vgg_in, m_nchw, (uint16_t*)d_fake, color, geo, flags, cut_h, cut_w,
              h, w, (const float*)ws, parts);
  CGAN_CHECK_LAUNCH("painter_heads_diffaug_bwd");
  return CGAN_OK;
}
