// The JPEG decoder's core (jpeg_decode.hip): plain functions on plain arrays, the same text for the host
// (cgan_jpeg_parse_host, cgan_jpeg_decode_coefficients_host: tested and run under sanitizers without a GPU) and for the kernels.
//
//   frame            the geometry a descriptor implies: MCUs, blocks per component, restart intervals
//   Bits             the bit reader: FF 00 un-stuffing, raw bit positions, never a byte at or behind the scan's end
//   decode_chunk     one subsequence from an entry state to its exit state, its symbols into a sink
//   CountSink        markers crossed, blocks begun and DC differences summed (what the prefix sum combines)
//   WriteSink        the coefficients to their places, every write inside the frame's block count
//   decode_serial    the rounds of the device taken one "thread" after the other (host twin)
//   idct_block       dequantisation and the fixed-point 8 x 8 inverse DCT
//   chroma_at / ycc_to_rgb   the triangle-filter upsampling and the 16-bit fixed-point colour conversion
//   parse            a file's bytes -> cgan_jpeg_desc (host only)
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "climategan_hip.h"
#include "jpeg_tables.h"

namespace jpeg_dec {

constexpr uint32_t DEFAULT_SUBSEQ = 128, MIN_SUBSEQ = 4, MAX_SUBSEQ = 4096;   // bytes of a subsequence
constexpr uint32_t MAX_SCAN_BYTES = 1u << 28;                                  // bit positions stay below 2^31

// ---- the frame -------------------------------------------------------------------------------------------------------------
// An MCU holds hs x vs luma blocks (raster order) and one block of each chroma component.  Coefficient layout: the components
// one after the other, each its blocks in raster order over the frame padded to whole MCUs, 64 values in natural order.
struct Frame {
  int ncomp, hs, vs, mcus_x, mcus_y, ny, bpm;
  int bw[3], bh[3];              // blocks per row / rows of blocks, per component
  int64_t off[3];                // first block of the component
  int64_t blocks, mcus, interval, nseg;   // interval: MCUs per restart interval (no DRI: all of them)
};
JPEG_HD inline Frame frame(const cgan_jpeg_desc& d) {
  Frame f;
  f.ncomp = d.ncomp, f.hs = d.hs, f.vs = d.vs;
  f.mcus_x = (d.width + 8 * d.hs - 1) / (8 * d.hs);
  f.mcus_y = (d.height + 8 * d.vs - 1) / (8 * d.vs);
  f.ny = d.hs * d.vs;
  f.bpm = f.ny + (d.ncomp == 3 ? 2 : 0);
  f.mcus = (int64_t)f.mcus_x * f.mcus_y;
  int64_t at = 0;
  for (int c = 0; c < 3; ++c) {
    f.bw[c] = c == 0 ? f.mcus_x * d.hs : (c < d.ncomp ? f.mcus_x : 0);
    f.bh[c] = c == 0 ? f.mcus_y * d.vs : (c < d.ncomp ? f.mcus_y : 0);
    f.off[c] = at;
    at += (int64_t)f.bw[c] * f.bh[c];
  }
  f.blocks = at;
  f.interval = d.restart_interval > 0 ? d.restart_interval : f.mcus;
  f.nseg = (f.mcus + f.interval - 1) / f.interval;
  return f;
}
// what the device calls and the host twin take: the ranges every index below relies on
JPEG_HD inline bool desc_ok(const cgan_jpeg_desc& d) {
  if (d.width < 1 || d.width > CGAN_JPEG_MAX_DIM || d.height < 1 || d.height > CGAN_JPEG_MAX_DIM) return false;
  if (d.ncomp != 1 && d.ncomp != 3) return false;
  if (!((d.hs == 1 && d.vs == 1) || (d.ncomp == 3 && d.hs == 2 && (d.vs == 1 || d.vs == 2)))) return false;
  if (d.restart_interval < 0 || d.restart_interval > 65535) return false;
  return d.scan_bytes <= MAX_SCAN_BYTES;
}
// block g of the scan (g = MCU * bpm + k) -> its index in the coefficient layout, and its component
JPEG_HD inline int64_t block_at(const Frame& f, int64_t g, int& comp) {
  const int64_t u = g / f.bpm;
  const int k = (int)(g % f.bpm);
  const int my = (int)(u / f.mcus_x), mx = (int)(u % f.mcus_x);
  if (k < f.ny) {
    comp = 0;
    return ((int64_t)my * f.vs + k / f.hs) * f.bw[0] + (int64_t)mx * f.hs + k % f.hs;
  }
  comp = k - f.ny + 1;
  return f.off[comp] + (int64_t)my * f.mcus_x + mx;
}
JPEG_HD inline uint32_t chunks_of(uint32_t scan_bytes, uint32_t subseq) { return scan_bytes == 0 ? 1u : (scan_bytes + subseq - 1) / subseq; }

// ---- the bit reader --------------------------------------------------------------------------------------------------------
// A position is a bit of the RAW scan (stuffed bytes included), so a state means the same to every thread.  `win` holds the
// next bits, most significant first, ones behind the last real bit; `n` of them are real.  A byte FF 00 enters as FF and
// marks in `skip` the depth at which the reader has passed it: taking bits across that depth moves the raw position 8 more.
// An FF followed by anything but 00, or the scan's end, ends the segment: nothing behind it is read.
struct Bits {
  const uint8_t* d;
  uint32_t len;
  uint64_t win, skip;
  int n;
  uint32_t pos, next, seg_end;
  bool ended;
  JPEG_HD void start(uint32_t p) {
    pos = p & ~7u, next = p >> 3, win = ~0ull, skip = 0, n = 0, ended = false, seg_end = len;
    fill();
    take(p & 7u);
  }
  JPEG_HD void fill() {
    while (!ended && n <= 56) {
      if (next >= len) {
        ended = true, seg_end = len;
        break;
      }
      const uint32_t b = d[next];
      if (b == 0xFFu) {
        if (next + 1 >= len || d[next + 1] != 0) {
          ended = true, seg_end = next;
          break;
        }
        skip |= 1ull << (56 - n);
        next += 2;
      } else {
        next += 1;
      }
      win = (win & ~(0xFFull << (56 - n))) | ((uint64_t)b << (56 - n));
      n += 8;
    }
  }
  JPEG_HD uint32_t peek(uint32_t k) const { return (uint32_t)(win >> (64u - k)); }        // 1 <= k <= 32
  JPEG_HD void take(uint32_t k) {                                                          // 0 <= k <= 32
    if (k == 0) return;
    pos += k + 8u * (uint32_t)__builtin_popcountll(skip >> (64u - k));
    skip <<= k;
    win = (win << k) | ((1ull << k) - 1ull);
    n -= (int)k;
  }
};

// the exit state of a subsequence: the raw bit position, the block within the MCU, the zig-zag position (0: a DC comes next)
struct State {
  uint32_t pos, bz;
};
JPEG_HD inline bool same(State a, State b) { return a.pos == b.pos && a.bz == b.bz; }
// the state nobody handed over: the subsequence's first byte that is not the second byte of a stuffed FF or of a marker
JPEG_HD inline State cold_state(const uint8_t* scan, uint32_t len, uint32_t subseq, uint32_t chunk) {
  uint32_t c = chunk * subseq;
  if (c > 0 && c < len && scan[c - 1] == 0xFFu) ++c;
  return State{8u * c, 0u};
}

struct Tables {
  const cgan_jpeg_hufftab* dc[3];
  const cgan_jpeg_hufftab* ac[3];
};
JPEG_HD inline int lookup(const cgan_jpeg_hufftab& t, uint32_t p16, uint32_t& len) {
  for (uint32_t l = 1; l <= 16; ++l)
    if (p16 < t.limit[l]) {
      len = l;
      return t.vals[((p16 >> (16u - l)) + (uint32_t)t.offset[l]) & 255u];
    }
  len = 16;
  return -1;
}
JPEG_HD inline int extend(uint32_t v, uint32_t s) { return v < (1u << (s - 1u)) ? (int)v - (int)(1u << s) + 1 : (int)v; }

// One subsequence: the bits [entry position, min((chunk + 1) * subseq, len) * 8) of the scan, symbol by symbol; a symbol
// belongs to the subsequence it begins in.  A segment ends where, on an MCU boundary, nothing or only 1 .. 7 one-bits are left
// (no code is all ones, so these cannot begin an MCU), or where no bit is left at all, which is corrupt inside an MCU as is a
// symbol that ran over the end.  There the sink is told and the decode goes on behind the marker with a fresh state.  `err` collects
// CGAN_JPEG_CORRUPT; it means something only when `in` is the true entry state.  At most 8 * subseq + 16 symbols: the loop
// ends whatever the bytes are.
template <typename Sink>
JPEG_HD inline State decode_chunk(const Tables& tb, const Frame& f, const uint8_t* scan, uint32_t len, uint32_t subseq,
                                  uint32_t chunk, uint32_t nchunks, State in, Sink& sink, uint32_t& err) {
  const uint64_t e64 = (uint64_t)(chunk + 1u) * subseq;
  // the last subsequence also owns the end of the scan itself: the last segment's end is checked by somebody
  const uint32_t end_bits = chunk + 1u >= nchunks || e64 >= len ? 8u * len + 1u : 8u * (uint32_t)e64;
  if (in.pos >= end_bits) return in;
  Bits r;
  r.d = scan, r.len = len;
  r.start(in.pos);
  uint32_t blk = in.bz >> 8, zz = in.bz & 255u;
  if (blk >= (uint32_t)f.bpm || zz > 63u) blk = 0, zz = 0;
  for (uint32_t it = 0; it < 8u * subseq + 16u && r.pos < end_bits; ++it) {
    r.fill();
    if (r.ended && (r.n <= 0 || (r.n < 8 && blk == 0 && zz == 0 && r.peek((uint32_t)r.n) == (1u << r.n) - 1u))) {
      if (r.n < 0 || blk != 0 || zz != 0) err |= CGAN_JPEG_CORRUPT;
      sink.cross(err);
      uint32_t j = r.seg_end;
      if (j >= len) {
        sink.finish(err);
        return State{8u * len + 8u, 0u};
      }
      while (j + 1 < len && scan[j + 1] == 0xFFu) ++j;          // fill bytes before the marker's code
      j = j + 2 < len ? j + 2 : len;
      r.start(8u * j);
      blk = 0, zz = 0;
      continue;
    }
    const int comp = blk < (uint32_t)f.ny ? 0 : (int)blk - f.ny + 1;
    uint32_t l;
    if (zz == 0) {
      int s = lookup(*tb.dc[comp], r.peek(16), l);
      if (s < 0 || s > 11) err |= CGAN_JPEG_CORRUPT, s = 0;
      r.take(l);
      int v = 0;
      if (s) v = extend(r.peek((uint32_t)s), (uint32_t)s), r.take((uint32_t)s);
      sink.begin(comp, v);
      zz = 1;
    } else {
      int rs = lookup(*tb.ac[comp], r.peek(16), l);
      if (rs < 0) err |= CGAN_JPEG_CORRUPT, rs = 0;
      r.take(l);
      const uint32_t run = (uint32_t)rs >> 4, s = (uint32_t)rs & 15u;
      if (s == 0) {
        if (run == 15u) {
          zz += 16;
        } else {
          if (run) err |= CGAN_JPEG_CORRUPT;
          zz = 64;
        }
      } else {
        zz += run;
        const int v = extend(r.peek(s), s);
        r.take(s);
        if (zz <= 63u) sink.ac((int)zz, v);
        zz += 1;
      }
      if (zz > 64u) err |= CGAN_JPEG_CORRUPT;
      if (zz >= 64u) zz = 0, blk = blk + 1u == (uint32_t)f.bpm ? 0u : blk + 1u;
    }
  }
  if (r.n < 0) err |= CGAN_JPEG_CORRUPT;       // the last symbol ran over its segment's end
  return State{r.pos, (blk << 8) | zz};
}

// What a subsequence adds to the running sums of its segment: the markers it crossed, the blocks begun and the DC differences
// summed behind the last of them (all of them if it crossed none).
struct Count {
  uint32_t m, b;
  int32_t dc[3];
};
JPEG_HD inline Count combine(const Count& a, const Count& c) {
  if (c.m) return Count{a.m + c.m, c.b, {c.dc[0], c.dc[1], c.dc[2]}};
  return Count{a.m, a.b + c.b, {a.dc[0] + c.dc[0], a.dc[1] + c.dc[1], a.dc[2] + c.dc[2]}};
}
struct CountSink {
  Count c{0, 0, {0, 0, 0}};
  JPEG_HD void begin(int comp, int diff) { c.dc[comp] += diff, c.b += 1; }
  JPEG_HD void ac(int, int) {}
  JPEG_HD void cross(uint32_t&) { c = Count{c.m + 1u, 0, {0, 0, 0}}; }
  JPEG_HD void finish(uint32_t&) {}
};
// The coefficients to their places.  `before`: the sums of all subsequences before this one.  Block number `bis` of segment
// `seg` is block seg * interval * bpm + bis of the scan; it is written only if the segment exists and has that many blocks.
struct WriteSink {
  const Frame& f;
  int16_t* coef;
  int64_t seg, bis;
  int32_t dc[3];
  int16_t* cur;
  JPEG_HD int64_t seg_blocks(int64_t s) const {
    const int64_t left = f.mcus - s * f.interval;
    return (left < f.interval ? left : f.interval) * f.bpm;
  }
  JPEG_HD int16_t* place(int64_t b, int& comp) const {
    comp = 0;
    if (seg >= f.nseg || b < 0 || b >= seg_blocks(seg)) return nullptr;
    return coef + 64 * block_at(f, seg * f.interval * f.bpm + b, comp);
  }
  JPEG_HD WriteSink(const Frame& fr, int16_t* co, const Count& before, State in)
      : f(fr), coef(co), seg(before.m), bis(before.b), dc{before.dc[0], before.dc[1], before.dc[2]}, cur(nullptr) {
    int comp;
    if ((in.bz & 255u) != 0) cur = place(bis - 1, comp);
  }
  JPEG_HD void begin(int, int diff) {
    int comp;
    cur = place(bis, comp);
    bis += 1;
    if (cur) dc[comp] += diff, cur[0] = (int16_t)dc[comp];
  }
  JPEG_HD void ac(int zz, int v) {
    if (cur) cur[jpeg_tab::zigzag(zz)] = (int16_t)v;
  }
  JPEG_HD void cross(uint32_t& err) {
    if (seg >= f.nseg || bis != seg_blocks(seg)) err |= CGAN_JPEG_CORRUPT;
    seg += 1, bis = 0, dc[0] = dc[1] = dc[2] = 0, cur = nullptr;
  }
  JPEG_HD void finish(uint32_t& err) {
    if (seg != f.nseg) err |= CGAN_JPEG_CORRUPT;
  }
};

JPEG_HD inline Tables tables_of(const cgan_jpeg_desc& d) {
  return Tables{{&d.dc[0], &d.dc[1], &d.dc[2]}, {&d.ac[0], &d.ac[1], &d.ac[2]}};
}

// The host twin: the rounds one "thread" after the other.  Round 1 decodes every subsequence from its cold state (the first
// from the scan's start); round r + 1 decodes subsequence i from the exit state subsequence i - 1 had after round r, if that
// changed.  After k rounds the first k subsequences are right by induction.  states / counts: nchunks entries of scratch.
// The write pass decodes once more from the states reached and checks that they are a fixpoint.  Returns the status;
// *rounds: the last round that changed a state.
inline uint32_t decode_serial(const cgan_jpeg_desc& d, const uint8_t* scan, uint32_t subseq, uint32_t round_cap, State* states,
                              State* entries, Count* counts, int16_t* coef, int32_t* rounds) {
  const Frame f = frame(d);
  const Tables tb = tables_of(d);
  const uint32_t len = d.scan_bytes, nchunks = chunks_of(len, subseq);
  uint32_t err = 0;
  auto run = [&](uint32_t i, State in) {
    CountSink sink;
    entries[i] = in;
    State out = decode_chunk(tb, f, scan, len, subseq, i, nchunks, in, sink, err);
    counts[i] = sink.c;
    return out;
  };
  for (uint32_t i = 0; i < nchunks; ++i) states[i] = run(i, i == 0 ? State{0, 0} : cold_state(scan, len, subseq, i));
  *rounds = 1;
  for (uint32_t r = 2; (round_cap == 0 || r <= round_cap) && r <= nchunks + 1; ++r) {
    bool changed = false;
    State prev = states[0];                     // the exit of i - 1 as the round before left it
    for (uint32_t i = 1; i < nchunks; ++i) {
      const State mine = states[i];
      if (!same(prev, entries[i])) {
        states[i] = run(i, prev);
        changed = changed || !same(states[i], mine);
      }
      prev = mine;
    }
    if (!changed) break;
    *rounds = (int32_t)r;
  }
  uint32_t status = 0;
  Count before{0, 0, {0, 0, 0}};
  for (uint32_t i = 0; i < nchunks; ++i) {
    const State in = i == 0 ? State{0, 0} : states[i - 1];
    if (!same(in, entries[i])) status |= CGAN_JPEG_NOT_CONVERGED;
    WriteSink sink(f, coef, before, in);
    uint32_t e = 0;
    const State out = decode_chunk(tb, f, scan, len, subseq, i, nchunks, in, sink, e);
    if (!same(out, states[i])) status |= CGAN_JPEG_NOT_CONVERGED;
    status |= e;
    before = combine(before, counts[i]);
  }
  return (status & CGAN_JPEG_NOT_CONVERGED) ? (uint32_t)CGAN_JPEG_NOT_CONVERGED : status;
}

// ---- reconstruction: all integer ------------------------------------------------------------------------------------------
// Dequantisation and the 8 x 8 inverse DCT of libjpeg's jidctint: 13-bit constants, the column pass keeps 2 extra bits, the
// row pass descales by 18, then + 128 and the clamp.  coef, quant: natural order; out: 64 samples, row-major.
JPEG_HD inline void idct8(const int32_t (&x)[8], int32_t (&y)[8], int shift) {
  constexpr int32_t F0_298 = 2446, F0_390 = 3196, F0_541 = 4433, F0_765 = 6270, F0_899 = 7373, F1_175 = 9633, F1_501 = 12299,
                    F1_847 = 15137, F1_961 = 16069, F2_053 = 16819, F2_562 = 20995, F3_072 = 25172;
  int32_t z1 = (x[2] + x[6]) * F0_541;
  const int32_t t2 = z1 - x[6] * F1_847, t3 = z1 + x[2] * F0_765;
  const int32_t t0 = (x[0] + x[4]) * 8192, t1 = (x[0] - x[4]) * 8192;
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int32_t o0 = x[7], o1 = x[5], o2 = x[3], o3 = x[1];
  z1 = o0 + o3;
  int32_t z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const int32_t z5 = (z3 + z4) * F1_175;
  o0 *= F0_298, o1 *= F2_053, o2 *= F3_072, o3 *= F1_501;
  z1 *= -F0_899, z2 *= -F2_562, z3 *= -F1_961, z4 *= -F0_390;
  z3 += z5, z4 += z5;
  o0 += z1 + z3, o1 += z2 + z4, o2 += z2 + z3, o3 += z1 + z4;
  const int32_t half = 1 << (shift - 1);
  y[0] = (t10 + o3 + half) >> shift, y[7] = (t10 - o3 + half) >> shift;
  y[1] = (t11 + o2 + half) >> shift, y[6] = (t11 - o2 + half) >> shift;
  y[2] = (t12 + o1 + half) >> shift, y[5] = (t12 - o1 + half) >> shift;
  y[3] = (t13 + o0 + half) >> shift, y[4] = (t13 - o0 + half) >> shift;
}
JPEG_HD inline void idct_block(const int16_t* coef, const uint8_t* quant, uint8_t* out) {
  int32_t ws[64];
  for (int c = 0; c < 8; ++c) {
    int32_t x[8], y[8];
    for (int r = 0; r < 8; ++r) x[r] = (int32_t)coef[8 * r + c] * (int32_t)quant[8 * r + c];
    idct8(x, y, 11);
    for (int r = 0; r < 8; ++r) ws[8 * r + c] = y[r];
  }
  for (int r = 0; r < 8; ++r) {
    int32_t x[8], y[8];
    for (int c = 0; c < 8; ++c) x[c] = ws[8 * r + c];
    idct8(x, y, 18);
    for (int c = 0; c < 8; ++c) {
      const int32_t v = y[c] + 128;
      out[8 * r + c] = (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
    }
  }
}
// The chroma sample of pixel (y, x) from a plane of `stride` bytes per row whose true extent is cw x ch: libjpeg's "fancy"
// triangle filter per halved direction (3/4 nearest, 1/4 next nearest, edges replicated); planes of at most 2 columns are
// replicated instead, as libjpeg does.
JPEG_HD inline int chroma_at(const uint8_t* p, int stride, int cw, int ch, int hs, int vs, int y, int x) {
  if (hs == 1) return p[(int64_t)y * stride + x];
  const int c = x >> 1;
  if (cw <= 2) return p[(int64_t)(vs == 2 ? y >> 1 : y) * stride + c];
  int cn = (x & 1) ? c + 1 : c - 1;
  cn = cn < 0 ? 0 : (cn > cw - 1 ? cw - 1 : cn);
  if (vs == 1) {
    const uint8_t* row = p + (int64_t)y * stride;
    return (3 * row[c] + row[cn] + ((x & 1) ? 2 : 1)) >> 2;
  }
  const int r = y >> 1;
  int rn = (y & 1) ? r + 1 : r - 1;
  rn = rn < 0 ? 0 : (rn > ch - 1 ? ch - 1 : rn);
  const uint8_t *r0 = p + (int64_t)r * stride, *r1 = p + (int64_t)rn * stride;
  const int near = 3 * r0[c] + r1[c], far = 3 * r0[cn] + r1[cn];
  return (3 * near + far + ((x & 1) ? 7 : 8)) >> 4;
}
// JFIF YCbCr -> RGB in libjpeg's 16-bit fixed point
JPEG_HD inline void ycc_to_rgb(int y, int cb, int cr, uint8_t* rgb) {
  cb -= 128, cr -= 128;
  const int r = y + ((91881 * cr + 32768) >> 16);
  const int g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
  const int b = y + ((116130 * cb + 32768) >> 16);
  rgb[0] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
  rgb[1] = (uint8_t)(g < 0 ? 0 : (g > 255 ? 255 : g));
  rgb[2] = (uint8_t)(b < 0 ? 0 : (b > 255 ? 255 : b));
}

// ---- the container (host only) -----------------------------------------------------------------------------------------------
struct RawHuff {
  bool set = false;
  uint8_t bits[16] = {0};
  uint8_t vals[256] = {0};
};
// Annex C, into the decode form; false if the lengths overfill the code space
inline bool build_hufftab(const RawHuff& h, cgan_jpeg_hufftab* t) {
  memset(t, 0, sizeof(*t));
  uint32_t code = 0, k = 0;
  for (uint32_t l = 1; l <= 16; ++l) {
    t->offset[l] = (int32_t)k - (int32_t)code;
    code += h.bits[l - 1], k += h.bits[l - 1];
    if (code > (1u << l)) return false;
    t->limit[l] = code << (16u - l);
    code <<= 1;
  }
  memcpy(t->vals, h.vals, 256);
  return true;
}

// One file's bytes -> *d.  Returns the status; `why` receives the reason of anything but OK.
inline int parse(const uint8_t* p, size_t n, cgan_jpeg_desc* d, char* why, size_t why_len) {
  auto fail = [&](int status, const char* text) {
    snprintf(why, why_len, "%s", text);
    return status;
  };
  memset(d, 0, sizeof(*d));
  if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) return fail(CGAN_JPEG_CORRUPT, "no SOI marker");
  uint8_t qt[4][64];
  bool qt_set[4] = {false, false, false, false};
  RawHuff huff[2][4];
  bool sof = false, adobe0 = false;
  int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0};
  size_t i = 2;
  for (;;) {
    if (i + 2 > n) return fail(CGAN_JPEG_CORRUPT, "the file ends before SOS");
    if (p[i] != 0xFF) return fail(CGAN_JPEG_CORRUPT, "a marker was expected");
    if (p[i + 1] == 0xFF) {               // a fill byte
      ++i;
      continue;
    }
    const int m = p[i + 1];
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7) || m == 0x00)
      return fail(CGAN_JPEG_CORRUPT, "a marker without a place among the headers");
    if (m == 0xD9) return fail(CGAN_JPEG_CORRUPT, "EOI before SOS");
    if (i + 4 > n) return fail(CGAN_JPEG_CORRUPT, "the file ends inside a segment's length");
    const size_t len = ((size_t)p[i + 2] << 8) | p[i + 3];
    if (len < 2 || i + 2 + len > n) return fail(CGAN_JPEG_CORRUPT, "a segment reaches behind the file's end");
    const uint8_t* s = p + i + 4;
    const size_t sl = len - 2;
    if (m == 0xC0) {
      if (sof) return fail(CGAN_JPEG_UNSUPPORTED, "several frames");
      if (sl < 6) return fail(CGAN_JPEG_CORRUPT, "SOF0 is too short");
      if (s[0] != 8) return fail(CGAN_JPEG_UNSUPPORTED, "samples of other than 8 bits");
      d->height = (s[1] << 8) | s[2], d->width = (s[3] << 8) | s[4];
      const int nc = s[5];
      if (d->height == 0) return fail(CGAN_JPEG_UNSUPPORTED, "height 0: the height comes in a DNL segment");
      if (d->width == 0) return fail(CGAN_JPEG_CORRUPT, "width 0");
      if (nc != 1 && nc != 3) return fail(CGAN_JPEG_UNSUPPORTED, "neither 1 nor 3 components (CMYK?)");
      if (sl != (size_t)(6 + 3 * nc)) return fail(CGAN_JPEG_CORRUPT, "SOF0 has the wrong length");
      if (d->width > CGAN_JPEG_MAX_DIM || d->height > CGAN_JPEG_MAX_DIM)
        return fail(CGAN_JPEG_UNSUPPORTED, "wider or higher than 8192");
      d->ncomp = nc;
      for (int c = 0; c < nc; ++c) {
        comp_id[c] = s[6 + 3 * c];
        const int h = s[7 + 3 * c] >> 4, v = s[7 + 3 * c] & 15;
        comp_tq[c] = s[8 + 3 * c];
        if (comp_tq[c] > 3) return fail(CGAN_JPEG_CORRUPT, "a quantisation table number above 3");
        if (h < 1 || h > 4 || v < 1 || v > 4) return fail(CGAN_JPEG_CORRUPT, "a sampling factor outside 1 .. 4");
        if (nc == 1) {
          d->hs = d->vs = 1;              // one component: its factors mean nothing
        } else if (c == 0) {
          if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2)))
            return fail(CGAN_JPEG_UNSUPPORTED, "luma sampling other than 1x1, 2x1, 2x2");
          d->hs = h, d->vs = v;
        } else if (h != 1 || v != 1) {
          return fail(CGAN_JPEG_UNSUPPORTED, "chroma sampling other than 1x1");
        }
      }
      if (nc == 3 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
        return fail(CGAN_JPEG_UNSUPPORTED, "RGB components");
      sof = true;
    } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4)) {
      return fail(CGAN_JPEG_UNSUPPORTED, m == 0xC2   ? "progressive"
                                         : m == 0xC1 ? "extended sequential"
                                         : m == 0xCC || m >= 0xC9 ? "arithmetic coding"
                                                                  : "lossless or hierarchical");
    } else if (m == 0xC4) {
      size_t at = 0;
      while (at < sl) {
        if (at + 17 > sl) return fail(CGAN_JPEG_CORRUPT, "DHT is cut");
        const int tc = s[at] >> 4, th = s[at] & 15;
        if (tc > 1 || th > 3) return fail(CGAN_JPEG_CORRUPT, "a Huffman table class or number out of range");
        RawHuff& h = huff[tc][th];
        size_t count = 0;
        for (int k = 0; k < 16; ++k) h.bits[k] = s[at + 1 + k], count += s[at + 1 + k];
        if (count > 256 || at + 17 + count > sl) return fail(CGAN_JPEG_CORRUPT, "DHT is cut");
        memset(h.vals, 0, 256);
        memcpy(h.vals, s + at + 17, count);
        h.set = true;
        at += 17 + count;
      }
    } else if (m == 0xDB) {
      size_t at = 0;
      while (at < sl) {
        if (s[at] >> 4) return fail(CGAN_JPEG_UNSUPPORTED, "16-bit quantisation table");
        const int tq = s[at] & 15;
        if (tq > 3) return fail(CGAN_JPEG_CORRUPT, "a quantisation table number above 3");
        if (at + 65 > sl) return fail(CGAN_JPEG_CORRUPT, "DQT is cut");
        for (int k = 0; k < 64; ++k) qt[tq][jpeg_tab::zigzag(k)] = s[at + 1 + k];
        qt_set[tq] = true;
        at += 65;
      }
    } else if (m == 0xDD) {
      if (sl != 2) return fail(CGAN_JPEG_CORRUPT, "DRI has the wrong length");
      d->restart_interval = (s[0] << 8) | s[1];
    } else if (m == 0xDC) {
      return fail(CGAN_JPEG_UNSUPPORTED, "DNL");
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(s, "Adobe", 5) == 0 && s[11] == 0) adobe0 = true;
    } else if (m == 0xDA) {
      if (!sof) return fail(CGAN_JPEG_CORRUPT, "SOS before SOF");
      if (sl < 1) return fail(CGAN_JPEG_CORRUPT, "SOS is too short");
      const int ns = s[0];
      if (ns != d->ncomp) return fail(CGAN_JPEG_UNSUPPORTED, "several scans (a scan without all components)");
      if (sl != (size_t)(4 + 2 * ns)) return fail(CGAN_JPEG_CORRUPT, "SOS has the wrong length");
      if (s[1 + 2 * ns] != 0 || s[2 + 2 * ns] != 63 || s[3 + 2 * ns] != 0)
        return fail(CGAN_JPEG_UNSUPPORTED, "a scan of part of the spectrum or with successive approximation");
      if (adobe0 && d->ncomp == 3) return fail(CGAN_JPEG_UNSUPPORTED, "Adobe APP14 segment with transform 0 (RGB)");
      for (int c = 0; c < ns; ++c) {
        if (s[1 + 2 * c] != comp_id[c]) return fail(CGAN_JPEG_UNSUPPORTED, "the scan's components are not in the frame's order");
        const int td = s[2 + 2 * c] >> 4, ta = s[2 + 2 * c] & 15;
        if (td > 3 || ta > 3 || !huff[0][td].set || !huff[1][ta].set) return fail(CGAN_JPEG_CORRUPT, "a Huffman table is missing");
        if (!build_hufftab(huff[0][td], &d->dc[c]) || !build_hufftab(huff[1][ta], &d->ac[c]))
          return fail(CGAN_JPEG_CORRUPT, "a Huffman table overfills its code space");
        if (!qt_set[comp_tq[c]]) return fail(CGAN_JPEG_CORRUPT, "a quantisation table is missing");
        memcpy(d->quant[c], qt[comp_tq[c]], 64);
      }
      i += 2 + len;
      break;
    }                                       // APPn, COM and everything else with a length: skipped
    i += 2 + len;
  }
  if (i > 0xFFFFFFFFu) return fail(CGAN_JPEG_UNSUPPORTED, "headers longer than 4 GiB");
  d->scan_offset = (uint32_t)i;
  // the entropy-coded data up to EOI: RSTm in their cycle, nothing else
  size_t j = i, end = n;
  uint32_t rst = 0;
  while (j < n) {
    const uint8_t* q = (const uint8_t*)memchr(p + j, 0xFF, n - j);
    if (!q) break;
    j = (size_t)(q - p);
    if (j + 1 >= n) {                      // the file ends on an FF: the data ends before it
      end = j;
      break;
    }
    const int m = p[j + 1];
    if (m == 0x00) {
      j += 2;
    } else if (m == 0xFF) {
      j += 1;
    } else if (m >= 0xD0 && m <= 0xD7) {
      if ((uint32_t)(m - 0xD0) != (rst & 7u)) return fail(CGAN_JPEG_CORRUPT, "restart markers out of their cycle");
      if (d->restart_interval == 0) return fail(CGAN_JPEG_CORRUPT, "a restart marker without a restart interval");
      ++rst;
      j += 2;
    } else if (m == 0xD9) {
      end = j;
      // fill bytes before EOI belong to the marker
      while (end > i && p[end - 1] == 0xFF) --end;
      break;
    } else if (m == 0xDC) {
      return fail(CGAN_JPEG_UNSUPPORTED, "DNL");
    } else {
      return fail(CGAN_JPEG_UNSUPPORTED, "several scans (a marker other than RSTm behind the scan)");
    }
  }
  if (end - i > MAX_SCAN_BYTES) return fail(CGAN_JPEG_UNSUPPORTED, "more than 256 MiB of entropy-coded data");
  d->scan_bytes = (uint32_t)(end - i);
  why[0] = 0;
  return CGAN_JPEG_OK;
}

}  // namespace jpeg_dec
