// PNG decoder on the device: a batch of files' zlib streams in one device blob -> one [h, w, c] image per file
// and one status word per file.  The parser (host), the bit reader, the code tables, the inflate step, the unfilter arithmetic
// and the Adler sums are png_decode_core.h: the kernels below call them, the host twin (cgan_png_decode_host) runs the same
// functions serially.
//
//   layout_kernel    one thread: every file's place in the workspace (a prefix sum over the files); for the row call also
//                    every candidate's place in the table of row offsets, and the "refused" words zeroed
//   inflate_kernel   one workgroup of one wave per file: the batch is the parallelism.  Lane 0 decodes up to 64 tokens into
//                    LDS (decode_tokens; the code tables are in LDS, the bit window in its registers); then the wave executes
//                    them in the stream's order (execute_tokens).  The last 32 KiB of output are kept in an LDS ring, which
//                    is all a match ever reads; the workspace is only written.  Leaves the stream's Adler-32 trailer.  Since
//                    DESIGN 4.24 the serial form: cgan_png_decode_lanes with subseq_bits = 0.
//   inflate_lanes_kernel  the same workgroup with the decode spread over the 64 lanes: inside a block of codes
//                    every lane decodes the tokens that begin in its subsequence of a window, first from its own first bit,
//                    again from its predecessor's exit bit until no entry changes; the committed lanes' tokens go through
//                    execute_tokens 64 at a time.  What cgan_png_decode and cgan_png_decode_rows' fallback launch.
//   unfilter_kernel  one workgroup of UNFILTER_WAVES waves per file, 64 rows per wave at a time as one skewed
//                    wavefront across the waves: lane r of a wave is at pixel t - r in the wave's step t, its left neighbour
//                    is its own last result, the two pixels above come from lane r - 1 by __shfl_up; lane 0 reads the row
//                    above from LDS, where lane 63 of the wave before left it.  Sums the Adler-32 of the bytes it reads
//                    anyway, row by row, and compares it with the trailer.  Writes the tight pixels.
// Launches and memsets per call: 1 memset (status) + layout + inflate + unfilter = 4.
//
// Row-framed files (cgan_png_decode_rows): files with one IDAT chunk per row, each row coded on its own and ended
// by a stored block on the chunk's last byte, as this project's encoder writes them (4.17).
//   inflate_rows_kernel  one workgroup of one wave per (row, file), the tail behind the last row as one more row.  The same
//                        shape as inflate_kernel -- lane 0 decodes up to 64 tokens (decode_tokens in MODE_ROW: the reader
//                        bounded to the row's chunk), the wave executes them -- with the row itself as the window, in dynamic
//                        LDS sized from the batch's longest row.  Whatever a row does not satisfy ORs the file's "refused" word.
//   inflate_lanes_kernel<true>  the whole-stream kernel for the files that are no candidates or were refused; the others'
//                        workgroups return.
// Launches and memsets per call: 1 memset (status) + layout + row inflate + serial inflate + unfilter = 5.  A row's reader
// ends with its chunk, and the table's offsets are checked on the host and again by the wave.
//
// Bounds: the reader never touches a byte outside [stream, stream + stream_bytes) (Reader::word); a stored run's source is
// checked against the stream's end (block_header); where a token's bytes go and what a match reads: see execute_tokens, the
// one place that writes inflated bytes.  Loops: a round of the serial kernels either brings 64 tokens, each of which consumed
// a bit, or is the last; the copies are bounded by a token's length, the wavefront by the image's size.  In the inflate
// kernels no wave waits for another: their barriers are __syncthreads() of a one-wave workgroup, reached by all lanes (every
// branch around them depends on values all lanes share).  The unfilter's waves do wait for each other, at barriers whose
// number comes from the descriptor alone (see unfilter_kernel).
#include "cgan_common.h"
#include "png_decode_host.h"

namespace {

using namespace png_dec;

constexpr int T = 64;                         // one wave
constexpr uint32_t BATCH = 64;                // tokens per round: one per lane
// the unfilter's workgroup: waves per file -- chosen from 4, 8 and 16 by measurement -- and the steps a wave
// runs behind its predecessor beyond the 64 that its rows lie lower
#ifndef CGAN_PNG_UNFILTER_WAVES
#define CGAN_PNG_UNFILTER_WAVES 16
#endif
constexpr int UNFILTER_WAVES = CGAN_PNG_UNFILTER_WAVES;
constexpr int UNFILTER_LAG = UNF_PREFETCH;

struct Workspace {
  uint64_t* layout;                           // per file: where its inflated bytes start in `inflated`
  uint32_t* adler;                            // per file: the trailer the stream had
  uint8_t* inflated;
  uint32_t* table_at;                         // the row calls only, per file: where its offsets start in the table; refused or not
  uint32_t* refused;
  size_t bytes;
};
inline size_t align16(size_t v) { return (v + 15) / 16 * 16; }
// the same arithmetic for the size query and the call
Workspace carve(void* base, const cgan_png_desc* descs, int32_t n, bool rows = false) {
  Workspace w;
  char* p = static_cast<char*>(base);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* q = p + at;
    at += align16(bytes);
    return q;
  };
  w.layout = reinterpret_cast<uint64_t*>(take(sizeof(uint64_t) * (size_t)n));
  w.adler = reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)n));
  size_t total = 0;
  for (int32_t i = 0; i < n; ++i) total += align16(inflated_bytes(descs[i]));
  w.inflated = reinterpret_cast<uint8_t*>(take(total));
  w.table_at = rows ? reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)n)) : nullptr;
  w.refused = rows ? reinterpret_cast<uint32_t*>(take(sizeof(uint32_t) * (size_t)n)) : nullptr;
  w.bytes = at;
  return w;
}

// w.table_at and w.refused: the row call's, null otherwise
__global__ void layout_kernel(const cgan_png_desc* __restrict__ descs, int n, Workspace w) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint64_t at = 0;
  uint32_t words = 0;
  for (int i = 0; i < n; ++i) {
    w.layout[i] = at;
    at += ((uint64_t)inflated_bytes(descs[i]) + 15) / 16 * 16;
    if (w.table_at) w.table_at[i] = words;
    words += table_words(descs[i]);
    if (w.refused) w.refused[i] = 0;
  }
}

// ---- the execute step ------------------------------------------------------------------------------------------------------
// The window a match reads: the bytes written so far, or the last of them, in LDS.  index(at): where byte `at` of the extent
// lives, always inside the buffer whatever `at` is.
struct RingWindow {                           // the last WINDOW bytes of a stream: uint8_t[WINDOW]
  uint8_t* base;
  __device__ uint32_t index(uint32_t at) const { return at & (WINDOW - 1); }
};
struct RowWindow {                            // a whole row of at most `cap` bytes: uint8_t[cap]
  uint8_t* base;
  uint32_t cap;
  __device__ uint32_t index(uint32_t at) const { return at % cap; }
};

// Up to 64 tokens, held one per lane (`have`: this lane holds one), appended at byte `pos` of an extent of `limit` bytes that
// starts at out[0]: a prefix sum over the tokens' lengths gives every token its place, each run of literals is scattered at
// once, each match or stored run is copied by all 64 lanes (a match whose distance is shorter than its length as a modular
// repeat), in the stream's order.  All lanes of a one-wave workgroup call it, with the same pos and limit; -> the new pos.
//   Bounds.  The commit's checks come first, wave-uniformly: a token must end inside the extent and a match must start at or
// behind out[0] (token_refused).  The tokens from the first refused one on are dropped and *refused is set: the caller ends
// its file as corrupt (or its row as refused) whatever its decoder's phase says.  decode_tokens has made the same checks for
// the serial kernels, where the verdict never comes; the lanes' windows are checked here alone.  So every write to `out` lies
// inside the extent, every index into the window goes through win.index, and a stored run reads stream bytes that
// block_header checked against the stream's end.
//   Order.  Nothing is written to the window ahead of its turn: a byte written early into the ring would take the slot of the
// byte 32 KiB before it, which a match still to come may read.  Hence the literals in front of a match are written, then a
// barrier, then the match reads and writes, then a barrier; the barriers stand under conditions all lanes share (ballots).
template <class Window>
__device__ inline uint32_t execute_tokens(Token k, bool have, uint32_t pos, uint32_t limit, Window win, uint8_t* __restrict__ out,
                                          const uint8_t* __restrict__ stream, bool* refused) {
  const uint32_t lane = threadIdx.x;
  if (!have) k = Token{0, 0, 0, 0};
  uint32_t incl = k.len;
  for (int off = 1; off < T; off <<= 1) {
    const uint32_t v = __shfl_up(incl, off);
    if ((int)lane >= off) incl += v;
  }
  const uint32_t mine = pos + incl - k.len;             // at most 64 * 65535 behind pos <= 2^29: no overflow
  const unsigned long long no = __ballot(have && (mine > limit || token_refused(k, mine, limit)));
  *refused = no != 0;
  if (no) have = have && (int)lane < __ffsll(no) - 1;   // the tokens in front of the first refused one are inside the extent
  if (!have) k = Token{0, 0, 0, 0};
  const uint32_t w0 = (uint32_t)k.len | ((uint32_t)k.kind << 16);
  unsigned long long todo = __ballot(have && k.kind != TOK_LITERAL);
  int done = -1;                                        // the tokens up to this one are executed
  while (todo) {                                        // at most 64 turns, the same in every lane
    const int i = __ffsll(todo) - 1;
    todo &= todo - 1;
    if (have && (int)lane > done && (int)lane < i) {    // literals all: the tokens between two set bits
      win.base[win.index(mine)] = k.lit;
      out[mine] = k.lit;
    }
    __syncthreads();
    const uint32_t m0 = __shfl(w0, i), arg = __shfl(k.arg, i), q = __shfl(mine, i);
    const uint32_t len = m0 & 0xFFFFu;
    if ((m0 >> 16) == TOK_MATCH) {
      const uint32_t from = q - arg;                    // arg <= q: token_refused
      for (uint32_t j = lane; j < len; j += T) {
        const uint8_t v = win.base[win.index(from + (arg < len ? j % arg : j))];
        win.base[win.index(q + j)] = v;
        out[q + j] = v;
      }
    } else {
      for (uint32_t j = lane; j < len; j += T) {        // arg + len <= the stream's (the chunk's) end: block_header checked it
        const uint8_t v = stream[arg + j];
        win.base[win.index(q + j)] = v;
        out[q + j] = v;
      }
    }
    __syncthreads();
    done = i;
  }
  if (have && (int)lane > done) {                       // the literals behind the last match
    win.base[win.index(mine)] = k.lit;
    out[mine] = k.lit;
  }
  const unsigned long long kept = __ballot(have);       // a prefix of the lanes
  const uint32_t total = kept ? __shfl(incl, 63 - __clzll(kept)) : 0u;
  __syncthreads();
  return pos + total;
}

// The prologue of the whole-stream kernels behind inflate_rows_kernel (cgan_png_decode_rows): writes the file's path -- 1: a
// candidate that no row refused, 0: not a candidate, 2: refused by the row path -- and -> whether the rows did the file, the
// same in every lane: the workgroup is done then.
__device__ inline bool done_by_rows(const cgan_png_desc& d, int file, const uint32_t* __restrict__ refused, int32_t* __restrict__ path) {
  const bool by_rows = d.rows != 0 && refused[file] == 0;
  if (threadIdx.x == 0) path[file] = by_rows ? 1 : (d.rows != 0 ? 2 : 0);
  return by_rows;
}

// One wave per (row, file): blockIdx.x = the row, or the file's height for the tail; blockIdx.y = the file.
//   table: the candidates' offsets one file behind the other, table_len words in all; cap: the bytes of `row`, at least the
//   longest 1 + row_bytes of the batch's candidates.
__global__ __launch_bounds__(T) void inflate_rows_kernel(const uint8_t* __restrict__ blob, const cgan_png_desc* __restrict__ descs,
                                                         const uint32_t* __restrict__ table, uint32_t table_len, Workspace w,
                                                         uint32_t cap) {
  extern __shared__ __align__(16) uint8_t row[];        // the row so far: all a match may read
  __shared__ Tables tables;
  __shared__ Token tok[BATCH];
  __shared__ uint32_t ctl[2];                 // tokens of the round; whether another round follows
  const int file = blockIdx.y;
  const uint32_t k = blockIdx.x, lane = threadIdx.x;
  const cgan_png_desc d = descs[file];
  if (d.rows == 0 || k > d.rows) return;                // the whole wave: not a candidate, or no such row
  const uint32_t t0 = w.table_at[file];
  const bool tail = k == d.rows;
  const uint32_t limit = tail ? 0u : 1u + row_bytes(d);
  // the chunk, checked once more where it is used: inside the table, ascending, inside the stream, the row inside the buffer
  uint32_t begin = 0, end = 0;
  bool ok = (uint64_t)t0 + d.rows + 1 <= table_len && limit <= cap;
  if (ok) {
    begin = table[t0 + k];
    end = tail ? d.stream_bytes : table[t0 + k + 1];
    ok = begin <= end && end <= d.stream_bytes;
  }
  if (!ok) {                                            // the same in every lane
    if (lane == 0) atomicOr(&w.refused[file], 1u);
    return;
  }
  const uint8_t* stream = blob + d.blob_offset;
  uint8_t* out = w.inflated + w.layout[file] + (size_t)(tail ? 0u : k) * limit;
  Inflate s;
  s.start_row(stream, begin, end, limit, tail ? MODE_TAIL : MODE_ROW);   // every lane the same; lane 0's is the one that advances
  uint32_t pos = 0;                                     // bytes executed so far, counted from the row's start; the same in every lane
  bool refused = false;                                 // the execute step's verdict, the same in every lane
  for (;;) {
    if (lane == 0) {
      ctl[0] = decode_tokens(s, tables, tok, BATCH);
      ctl[1] = (s.phase != PHASE_DONE && !s.err) ? 1u : 0u;
    }
    __syncthreads();
    const uint32_t nt = ctl[0] < BATCH ? ctl[0] : BATCH;
    const bool more = ctl[1] != 0 && nt == BATCH;       // a round that is not full is the last one
    pos = execute_tokens(tok[lane], lane < nt, pos, limit, RowWindow{row, cap}, out, stream, &refused);
    if (!more || refused) break;
  }
  if (lane == 0) {
    if (refused || s.err || s.phase != PHASE_DONE) atomicOr(&w.refused[file], 1u);
    else if (tail) w.adler[file] = s.adler;
  }
}

// PREDICATED (cgan_png_decode_rows): behind inflate_rows_kernel, for the files the rows did not do (done_by_rows).
template <bool PREDICATED>
__global__ __launch_bounds__(T) void inflate_kernel(const uint8_t* __restrict__ blob, const cgan_png_desc* __restrict__ descs,
                                                    Workspace w, int32_t* __restrict__ status, int32_t* __restrict__ path) {
  __shared__ Tables tables;
  __shared__ Token tok[BATCH];
  __shared__ uint32_t ctl[2];                 // tokens of the round; whether another round follows
  __shared__ uint8_t ring[WINDOW];
  const int file = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const cgan_png_desc d = descs[file];
  if constexpr (PREDICATED) {
    if (done_by_rows(d, file, w.refused, path)) return;
  }
  const uint8_t* stream = blob + d.blob_offset;
  uint8_t* out = w.inflated + w.layout[file];
  const uint32_t limit = inflated_bytes(d);
  Inflate s;
  s.start(stream, d.stream_bytes, limit);               // every lane the same; lane 0's is the one that advances
  uint32_t pos = 0;                                     // bytes executed so far, the same in every lane
  bool refused = false;                                 // the execute step's verdict, the same in every lane
  for (;;) {
    if (lane == 0) {
      ctl[0] = decode_tokens(s, tables, tok, BATCH);
      ctl[1] = (s.phase != PHASE_DONE && !s.err) ? 1u : 0u;
    }
    __syncthreads();
    const uint32_t nt = ctl[0] < BATCH ? ctl[0] : BATCH;
    const bool more = ctl[1] != 0 && nt == BATCH;       // a round that is not full is the last one
    pos = execute_tokens(tok[lane], lane < nt, pos, limit, RingWindow{ring}, out, stream, &refused);
    if (!more || refused) break;
  }
  if (lane == 0) {
    if (refused || s.err || s.phase != PHASE_DONE) atomicOr(&status[file], (int32_t)CGAN_PNG_CORRUPT);
    w.adler[file] = s.adler;
  }
}

// ---- the inflate across the wave's lanes ----------------------------------------------------------------------
// One workgroup of one wave per file, as inflate_kernel.  Lane 0 owns the stream's state (Inflate) and reads block headers,
// stored blocks and the trailer serially (phase_step); inside a block of codes the wave decodes windows of 64 * S bits by the
// window rule of png_decode_core.h -- every lane its subsequence into its own LDS slots, again from its predecessor's exit bit
// until no entry changes -- and commits the lanes up to the first that did not run to its range's end: their tokens pass
// through execute_tokens 64 at a time, in the stream's order.  A token of a lane that is not committed is never read.
// Every barrier stands under conditions all lanes share (ctl[], ballots, shuffled values); none inside the per-lane decode.
// Loops: the passes are counted to 64, a lane's tokens to `cap`, a window's commit to 64 * cap tokens, and every window or
// serial step consumes a bit of the stream or ends the file.  Slots, tables and ring are indexed through slot_index, masks
// and the sizes of their arrays; the readers never leave the stream.
template <bool PREDICATED>
__global__ __launch_bounds__(T) void inflate_lanes_kernel(const uint8_t* __restrict__ blob, const cgan_png_desc* __restrict__ descs,
                                                          Workspace w, int32_t* __restrict__ status, int32_t* __restrict__ path,
                                                          uint32_t S, uint32_t cap) {
  __shared__ Tables tables;
  __shared__ Token slot[LANES * LANE_SLOTS];
  __shared__ Token tok[BATCH];
  __shared__ uint32_t ctl[3];                 // stored tokens of the serial step; what follows; the bit the window starts at
  __shared__ uint16_t base[LANES + 1];        // the committed lanes' tokens: lane i's are base[i] .. base[i + 1]
  __shared__ uint8_t ring[WINDOW];
  const int file = blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const cgan_png_desc d = descs[file];
  if constexpr (PREDICATED) {
    if (done_by_rows(d, file, w.refused, path)) return;
  }
  const uint8_t* stream = blob + d.blob_offset;
  uint8_t* out = w.inflated + w.layout[file];
  const uint32_t limit = inflated_bytes(d);
  const RingWindow win{ring};
  if (cap > LANE_SLOTS) cap = LANE_SLOTS;
  Inflate s;
  s.start(stream, d.stream_bytes, limit);               // every lane the same; lane 0's is the one that advances
  uint32_t pos = 0;                                     // bytes executed so far, the same in every lane
  bool corrupt = false;                                 // found at a commit, the same in every lane
  constexpr uint32_t ENDED = 0, SERIAL = 1, CODES = 2;
  for (;;) {
    // the serial phases, lane 0: up to BATCH steps, each of which consumes stream or ends the file
    if (lane == 0) {
      uint32_t nt = 0, steps = 0;
      s.out = pos;
      while (s.phase != PHASE_CODES && s.phase != PHASE_DONE && !s.err && steps++ < BATCH) nt = phase_step(s, tables, tok, nt);
      ctl[0] = nt;
      ctl[1] = (s.phase == PHASE_DONE || s.err) ? ENDED : (s.phase == PHASE_CODES ? CODES : SERIAL);
      ctl[2] = (uint32_t)s.r.used();
    }
    __syncthreads();
    const uint32_t nt = ctl[0] < BATCH ? ctl[0] : BATCH, next = ctl[1];
    uint32_t P = ctl[2];
    bool refused;
    pos = execute_tokens(tok[lane], lane < nt, pos, limit, win, out, stream, &refused);      // stored runs: checked by phase_step
    corrupt = refused;
    if (next == ENDED || corrupt) break;
    if (next == SERIAL) continue;
    // windows, until one commits an end-of-block symbol, an invalid symbol or a refused token
    uint32_t flag = SUB_NONE;
    while (flag != SUB_EOB) {
      uint32_t entry = lane_first_entry(P, lane, S);
      const uint32_t end = lane_end(P, lane, S);
      SubExit ex{entry, SUB_NONE, 0};
      bool changed = true;
      for (uint32_t pass = 0; pass < LANES; ++pass) {
        if (changed) ex = entry >= end ? SubExit{entry, SUB_NONE, 0} : decode_subseq(stream, d.stream_bytes, entry, tables, end, slot, lane, cap);
        const uint32_t before = __shfl_up(ex.bit, 1), before_flag = __shfl_up(ex.flag, 1);
        changed = lane > 0 && before_flag == SUB_NONE && before != entry;
        if (changed) entry = before;
        if (!__any(changed)) break;
      }
      const unsigned long long stopped = __ballot(ex.flag != SUB_NONE);
      const int c = stopped ? __ffsll(stopped) - 1 : (int)LANES - 1;
      flag = __shfl(ex.flag, c);
      P = __shfl(ex.bit, c);
      const uint32_t count = (int)lane <= c ? (ex.count < cap ? ex.count : cap) : 0u;
      uint32_t incl = count;
      for (int off = 1; off < T; off <<= 1) {
        const uint32_t v = __shfl_up(incl, off);
        if ((int)lane >= off) incl += v;
      }
      if (lane == 0) base[0] = 0;
      base[lane + 1] = (uint16_t)incl;                  // at most 64 * LANE_SLOTS
      const uint32_t total = __shfl(incl, T - 1);
      __syncthreads();                                  // the slots and base[] are written
      for (uint32_t g0 = 0; g0 < total && !corrupt; g0 += BATCH) {
        const uint32_t g = g0 + lane;
        const bool have = g < total;
        uint32_t l = 0;                                 // the lane whose tokens hold token g: base[l] <= g < base[l + 1]
        for (uint32_t step = LANES / 2; step; step >>= 1)
          if (base[l + step] <= g) l += step;
        Token k{0, 0, 0, 0};
        if (have) k = slot[slot_index(l, g - base[l])];
        pos = execute_tokens(k, have, pos, limit, win, out, stream, &refused);
        corrupt = refused;
      }
      __syncthreads();                                  // the slots are read before the next window writes them
      if (flag == SUB_BAD) corrupt = true;
      if (corrupt) break;
    }
    if (corrupt) break;
    if (lane == 0) {                                    // behind the end-of-block symbol: the next header, or the trailer
      s.r.seat_bit(P);
      s.phase = s.last ? PHASE_TRAILER : PHASE_HEADER;
    }
  }
  if (lane == 0) {
    if (corrupt || s.err || s.phase != PHASE_DONE) atomicOr(&status[file], (int32_t)CGAN_PNG_CORRUPT);
    w.adler[file] = s.adler;
  }
}

// One workgroup of NW waves per file (the schedule is png_decode_core.h's unf_* functions, which the host twin
// host_unfilter_wide runs step by step).  Inside a wave: a skewed wavefront, lane r at pixel t - r in the wave's step t, the left
// neighbour its own last result, the two pixels above from lane r - 1 by __shfl_up.  Between waves: wave j runs j * (64 + LAG)
// steps behind wave 0; its lane 0 reads the row above from ring[j], where lane 63 of wave j - 1 wrote it LAG + 1 steps -- at
// least one barrier -- earlier.  Between passes: lane 63 of the last wave leaves its row in `above` for wave 0.
// Every loop around a barrier counts chunks and passes, which come from the descriptor: all waves and lanes make the same
// turns, and those with no row or no pixel only skip the memory accesses.  The one early return is the same in every thread.
template <int NW, int LAG>
__global__ __launch_bounds__(T * NW) void unfilter_kernel(const cgan_png_desc* __restrict__ descs, Workspace w,
                                                          uint8_t* __restrict__ out_base, int32_t* __restrict__ status) {
  static_assert(NW >= 1 && NW <= UNF_MAX_WAVES && LAG >= UNF_PREFETCH && LAG % UNF_PREFETCH == 0, "see unf_params_ok");
  constexpr uint32_t RING = unf_ring_words(LAG);
  __shared__ uint32_t above[CGAN_PNG_MAX_DIM];          // the last row of the pass before, a pixel per word
  __shared__ uint32_t ring[NW][RING];                   // ring[j]: the last row of wave j - 1, the pixels wave j reads next
  __shared__ uint32_t sums[NW][3];                      // per wave: the Adler sums of its rows, whether a filter byte was bad
  __shared__ int32_t skip;
  const int file = blockIdx.x;
  const int wave = threadIdx.x / T, lane = threadIdx.x % T;
  if (threadIdx.x == 0) skip = status[file];
  __syncthreads();
  if (skip != 0) return;                                // every thread: the inflate failed, there is nothing to unfilter
  const cgan_png_desc d = descs[file];
  const int W = d.width, H = d.height;
  const uint32_t bpp = bytes_per_pixel(d), rb = row_bytes(d), total = inflated_bytes(d);
  const bool swap = d.bit_depth == 16;
  const uint8_t* in = w.inflated + w.layout[file];
  uint8_t* out = out_base + d.out_offset;
  const uint32_t passes = unf_passes(H, NW), chunks = unf_chunks(W, NW, LAG);
  const int behind = unf_wave_offset(wave, LAG);
  Adler ad;
  ad.start();
  bool bad = false;
  for (uint32_t p = 0; p < passes; ++p) {
    const int y = unf_row(p, wave, lane, NW);
    const bool live = y < H;
    const uint8_t* row = in + (size_t)(live ? y : 0) * (1 + rb);
    const uint32_t filter = live ? row[0] : 0u;
    if (live) ad.byte(filter);
    bad = bad || filter > 4;
    uint32_t cur = 0, prev = 0, above_left = 0;         // my results of the last step and the one before; lane 0: its last b
    for (uint32_t c = 0; c < chunks; ++c) {
      const int t0 = (int)(c * UNF_PREFETCH) - behind;
      if (!unf_wave_idle(unf_row(p, wave, 0, NW), H, t0, W)) {             // the same in every lane of the wave; no barrier inside
        uint32_t raw[UNF_PREFETCH];
#pragma unroll
        for (int u = 0; u < UNF_PREFETCH; ++u) {
          const int x = t0 + u - lane;
          raw[u] = 0;
          if (live && x >= 0 && x < W)
            for (uint32_t k = 0; k < bpp; ++k) raw[u] |= (uint32_t)row[1 + (uint32_t)x * bpp + k] << (8 * k);
        }
#pragma unroll
        for (int u = 0; u < UNF_PREFETCH; ++u) {
          const int x = t0 + u - lane;
          const bool active = live && x >= 0 && x < W;
          uint32_t b = __shfl_up(cur, 1), cc = __shfl_up(prev, 1);
          if (lane == 0) {
            cc = above_left;
            b = 0u;
            if (active) {
              if (wave > 0) b = ring[wave][unf_ring_index(x, RING)];
              else if (p > 0) b = above[unf_above_index(x)];
            }
            above_left = b;
          }
          const uint32_t v = active ? unfilter_pixel(filter, raw[u], cur, b, cc) : 0u;
          if (active) {
            uint8_t* px = out + ((size_t)y * W + x) * bpp;
            for (uint32_t k = 0; k < bpp; ++k) {
              px[swap ? 1 - k : k] = (uint8_t)(v >> (8 * k));
              ad.byte((raw[u] >> (8 * k)) & 255u);
            }
            if (lane == T - 1) {
              if (wave + 1 < NW) ring[(wave + 1) % NW][unf_ring_index(x, RING)] = v;
              else above[unf_above_index(x)] = v;
            }
          }
          prev = cur, cur = v;
        }
      }
      __syncthreads();                                  // chunks * passes of them, whatever the wave and the lane
    }
    if (live) ad.end_piece(total - (uint32_t)(y + 1) * (1 + rb));
  }
  uint32_t s1 = ad.s1, s2 = ad.s2;
  for (int off = 1; off < T; off <<= 1) {
    s1 = (s1 + __shfl_xor(s1, off)) % ADLER_MOD;
    s2 = (s2 + __shfl_xor(s2, off)) % ADLER_MOD;
  }
  const bool any_bad = __ballot(bad) != 0;
  if (lane == 0) sums[wave][0] = s1, sums[wave][1] = s2, sums[wave][2] = any_bad ? 1u : 0u;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t flag = 0;
    s1 = 0, s2 = 0;
    for (int j = 0; j < NW; ++j) {
      s1 = (s1 + sums[j][0]) % ADLER_MOD;
      s2 = (s2 + sums[j][1]) % ADLER_MOD;
      flag |= sums[j][2];
    }
    if (flag || adler_value(s1, s2, total) != w.adler[file]) atomicOr(&status[file], (int32_t)CGAN_PNG_CORRUPT);
  }
}

void launch_unfilter(int32_t n, hipStream_t s, const cgan_png_desc* descs_dev, const Workspace& w, uint8_t* out, int32_t* status) {
  hipLaunchKernelGGL((unfilter_kernel<UNFILTER_WAVES, UNFILTER_LAG>), dim3(n), dim3(T * UNFILTER_WAVES), 0, s, descs_dev, w, out, status);
}

int descs_ok(const char* what, const cgan_png_desc* descs, int32_t n, size_t blob_bytes, bool with_out, size_t out_bytes) {
  CGAN_REQUIRE(descs, "%s: null pointer", what);
  CGAN_REQUIRE(n >= 1 && n <= 65535, "%s: n = %d: 1 <= n <= 65535 expected", what, n);
  for (int32_t i = 0; i < n; ++i) {
    const cgan_png_desc& d = descs[i];
    CGAN_REQUIRE(desc_ok(d), "%s: descriptor %d is not one the parser produces", what, i);
    CGAN_REQUIRE(d.blob_offset >= 0 && d.blob_offset % 4 == 0 && (uint64_t)d.blob_offset + d.stream_bytes <= blob_bytes,
                 "%s: the stream of file %d is not 4-byte aligned or reaches behind the blob's end", what, i);
    if (with_out)
      CGAN_REQUIRE(d.out_offset >= 0 && d.out_offset % (d.bit_depth / 8) == 0 &&
                       (uint64_t)d.out_offset + pixel_bytes(d) <= out_bytes,
                   "%s: the pixels of file %d are misaligned or reach behind the output's end", what, i);
  }
  return CGAN_OK;
}

}  // namespace

extern "C" int cgan_png_parse_host(const uint8_t* file, size_t file_bytes, cgan_png_desc* desc, int32_t* status) {
  char why[160] = "";
  const int rc = host_parse(file, file_bytes, desc, status, why, sizeof(why));
  if (rc || *status) cgan_set_error("cgan_png_parse_host: %s", why);
  return rc ? CGAN_ERR_BAD_ARG : CGAN_OK;
}

extern "C" int cgan_png_stream_host(const uint8_t* file, size_t file_bytes, const cgan_png_desc* desc, uint8_t* dst,
                                    size_t dst_bytes) {
  char why[160] = "";
  const int rc = host_stream(file, file_bytes, desc, dst, dst_bytes, why, sizeof(why));
  if (rc) cgan_set_error("cgan_png_stream_host: %s", why);
  return rc ? CGAN_ERR_BAD_ARG : CGAN_OK;
}

extern "C" int cgan_png_decode_host(const uint8_t* stream, const cgan_png_desc* desc, uint8_t* inflated, uint8_t* pixels,
                                    int32_t* status) {
  char why[160] = "";
  const int rc = host_decode(stream, desc, inflated, pixels, status, why, sizeof(why));
  if (rc || *status) cgan_set_error("cgan_png_decode_host: %s", why);
  return rc ? CGAN_ERR_BAD_ARG : CGAN_OK;
}

extern "C" void cgan_png_unfilter_wide_params(int32_t* waves, int32_t* lag, int32_t* prefetch) {
  if (waves) *waves = UNFILTER_WAVES;
  if (lag) *lag = UNFILTER_LAG;
  if (prefetch) *prefetch = UNF_PREFETCH;
}

extern "C" int cgan_png_unfilter_wide_host(const cgan_png_desc* desc, const uint8_t* inflated, uint32_t trailer, int32_t waves,
                                           int32_t lag, uint8_t* pixels, int32_t* status) {
  char why[160] = "";
  if (!desc) {
    cgan_set_error("cgan_png_unfilter_wide_host: null pointer");
    return CGAN_ERR_BAD_ARG;
  }
  const int rc = host_unfilter_wide(*desc, inflated, trailer, waves, lag, pixels, status, why, sizeof(why));
  if (rc || *status) cgan_set_error("cgan_png_unfilter_wide_host: %s", why);
  return rc == 0 ? CGAN_OK : (rc == -2 ? CGAN_ERR_INTERNAL : CGAN_ERR_BAD_ARG);
}

extern "C" size_t cgan_png_decode_workspace_bytes(const cgan_png_desc* descs_host, int32_t n) {
  if (descs_ok("cgan_png_decode_workspace_bytes", descs_host, n, ~(size_t)0, false, 0)) return 0;
  return carve(nullptr, descs_host, n).bytes;
}

namespace {

// the whole-stream inflate in its two forms: subseq_bits = 0 the serial kernel, else the lanes' windows
template <bool PREDICATED>
void launch_inflate(int32_t n, hipStream_t s, const uint8_t* blob, const cgan_png_desc* descs_dev, const Workspace& w, int32_t* status,
                    int32_t* path, int32_t subseq_bits, int32_t lane_tokens) {
  if (subseq_bits == 0)
    hipLaunchKernelGGL(inflate_kernel<PREDICATED>, dim3(n), dim3(T), 0, s, blob, descs_dev, w, status, path);
  else
    hipLaunchKernelGGL(inflate_lanes_kernel<PREDICATED>, dim3(n), dim3(T), 0, s, blob, descs_dev, w, status, path, (uint32_t)subseq_bits,
                       (uint32_t)lane_tokens);
}

// The host half of the row path: the descriptors as cgan_png_decode checks them, and the candidates' tables one
// file behind the other.  *max_rows / *cap: the grid's width and the row buffer's bytes.
int rows_ok(const char* what, const cgan_png_desc* descs, const uint32_t* tables, size_t table_len, int32_t n, size_t blob_bytes,
            bool with_out, size_t out_bytes, uint32_t* max_rows, uint32_t* cap) {
  if (const int rc = descs_ok(what, descs, n, blob_bytes, with_out, out_bytes)) return rc;
  size_t at = 0;
  *max_rows = 0, *cap = 16;
  for (int32_t i = 0; i < n; ++i) {
    const cgan_png_desc& d = descs[i];
    if (d.rows == 0) continue;
    CGAN_REQUIRE(tables && at + d.rows + 1 <= table_len, "%s: the table ends before the offsets of file %d", what, i);
    CGAN_REQUIRE(table_ok(d, tables + at),
                 "%s: the offsets of file %d do not start behind the zlib header, ascend and stay inside its stream", what, i);
    at += d.rows + 1;
    if (d.rows > *max_rows) *max_rows = d.rows;
    const uint32_t need = (1u + row_bytes(d) + 15u) / 16u * 16u;
    if (need > *cap) *cap = need;
  }
  CGAN_REQUIRE(at == table_len, "%s: a table of %zu words for descriptors whose rows need %zu", what, table_len, at);
  return CGAN_OK;
}

// what cgan_png_decode_rows has beyond cgan_png_decode: the candidates' row tables and where every file's path goes
struct RowPart {
  const uint32_t *tables_host, *tables_dev;
  size_t table_len;
  int32_t* path;
};

// The one body of cgan_png_decode, cgan_png_decode_lanes and cgan_png_decode_rows (rows: the last one's, else null): the
// checks, the workspace, the memset and the launches -- with rows the table's checks, the row launch in front of the
// whole-stream one, and that one predicated.
int png_decode_impl(const char* what, const uint8_t* blob, size_t blob_bytes, const cgan_png_desc* descs_host,
                    const cgan_png_desc* descs_dev, const RowPart* rows, int32_t n, uint8_t* out, size_t out_bytes, int32_t* status,
                    void* workspace, size_t workspace_bytes, void* stream, int32_t subseq_bits, int32_t lane_tokens) {
  CGAN_REQUIRE(lanes_params_ok(subseq_bits, lane_tokens),
               "%s: subseq_bits = %d, lane_tokens = %d: 0 or a multiple of 32 up to %u, and 1 .. %u, expected", what, subseq_bits,
               lane_tokens, SUBSEQ_BITS_MAX, LANE_SLOTS);
  CGAN_REQUIRE(blob && descs_dev && out && status && workspace && (!rows || rows->path), "%s: null pointer", what);
  uint32_t max_rows = 0, cap = 0;
  if (const int rc = rows ? rows_ok(what, descs_host, rows->tables_host, rows->table_len, n, blob_bytes, true, out_bytes, &max_rows, &cap)
                          : descs_ok(what, descs_host, n, blob_bytes, true, out_bytes))
    return rc;
  CGAN_REQUIRE(!rows || rows->table_len == 0 || rows->tables_dev, "%s: null pointer", what);
  CGAN_REQUIRE(reinterpret_cast<uintptr_t>(blob) % 4 == 0, "%s: the blob is not 4-byte aligned", what);
  CGAN_REQUIRE(!rows || reinterpret_cast<uintptr_t>(rows->tables_dev) % 4 == 0, "%s: the table is not 4-byte aligned", what);
  CGAN_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: the workspace is not 16-byte aligned", what);
  const Workspace w = carve(workspace, descs_host, n, rows != nullptr);
  if (w.bytes > workspace_bytes) {
    cgan_set_error("%s: the workspace has %zu bytes, %zu are needed", what, workspace_bytes, w.bytes);
    return CGAN_ERR_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)n, s) != hipSuccess) {
    cgan_set_error("%s: hipMemsetAsync failed", what);
    return CGAN_ERR_HIP;
  }
  hipLaunchKernelGGL(layout_kernel, dim3(1), dim3(64), 0, s, descs_dev, n, w);
  CGAN_CHECK_LAUNCH(rows ? "cgan_png_decode_rows (layout)" : "cgan_png_decode (layout)");
  if (max_rows) {
    hipLaunchKernelGGL(inflate_rows_kernel, dim3(max_rows + 1, n), dim3(T), cap, s, blob, descs_dev, rows->tables_dev,
                       (uint32_t)rows->table_len, w, cap);
    CGAN_CHECK_LAUNCH("cgan_png_decode_rows (rows)");
  }
  if (rows) launch_inflate<true>(n, s, blob, descs_dev, w, status, rows->path, subseq_bits, lane_tokens);
  else launch_inflate<false>(n, s, blob, descs_dev, w, status, nullptr, subseq_bits, lane_tokens);
  CGAN_CHECK_LAUNCH(rows ? "cgan_png_decode_rows (inflate)" : "cgan_png_decode (inflate)");
  launch_unfilter(n, s, descs_dev, w, out, status);
  CGAN_CHECK_LAUNCH(rows ? "cgan_png_decode_rows (unfilter)" : "cgan_png_decode (unfilter)");
  return CGAN_OK;
}

}  // namespace

extern "C" int cgan_png_decode(const uint8_t* blob, size_t blob_bytes, const cgan_png_desc* descs_host,
                               const cgan_png_desc* descs_dev, int32_t n, uint8_t* out, size_t out_bytes, int32_t* status,
                               void* workspace, size_t workspace_bytes, void* stream) {
  return png_decode_impl("cgan_png_decode", blob, blob_bytes, descs_host, descs_dev, nullptr, n, out, out_bytes, status, workspace,
                         workspace_bytes, stream, (int32_t)SUBSEQ_BITS_DEFAULT, (int32_t)LANE_TOKENS_DEFAULT);
}

extern "C" int cgan_png_decode_lanes(const uint8_t* blob, size_t blob_bytes, const cgan_png_desc* descs_host,
                                     const cgan_png_desc* descs_dev, int32_t n, uint8_t* out, size_t out_bytes, int32_t* status,
                                     void* workspace, size_t workspace_bytes, void* stream, int32_t subseq_bits, int32_t lane_tokens) {
  return png_decode_impl("cgan_png_decode_lanes", blob, blob_bytes, descs_host, descs_dev, nullptr, n, out, out_bytes, status,
                         workspace, workspace_bytes, stream, subseq_bits, lane_tokens);
}

extern "C" void cgan_png_inflate_lanes_params(int32_t* subseq_bits, int32_t* lane_tokens) {
  if (subseq_bits) *subseq_bits = (int32_t)SUBSEQ_BITS_DEFAULT;
  if (lane_tokens) *lane_tokens = (int32_t)LANE_TOKENS_DEFAULT;
}

extern "C" int cgan_png_inflate_lanes_host(const uint8_t* stream, const cgan_png_desc* desc, int32_t subseq_bits, int32_t lane_tokens,
                                           uint8_t* inflated, uint32_t* trailer, uint32_t* stats, int32_t* status) {
  char why[200] = "";
  const int rc = host_inflate_lanes(stream, desc, subseq_bits, lane_tokens, inflated, trailer, stats, status, why, sizeof(why));
  if (rc || *status) cgan_set_error("cgan_png_inflate_lanes_host: %s", why);
  return rc ? CGAN_ERR_BAD_ARG : CGAN_OK;
}

// ---- row-framed files ------------------------------------------------------------------------------------
extern "C" int cgan_png_row_table_host(const uint8_t* file, size_t file_bytes, const cgan_png_desc* desc, uint32_t* table) {
  char why[160] = "";
  const int rc = host_row_table(file, file_bytes, desc, table, why, sizeof(why));
  if (rc) cgan_set_error("cgan_png_row_table_host: %s", why);
  return rc ? CGAN_ERR_BAD_ARG : CGAN_OK;
}

extern "C" int cgan_png_decode_rows_host(const uint8_t* stream, const cgan_png_desc* desc, const uint32_t* table, uint8_t* inflated,
                                         uint8_t* pixels, int32_t* status, int32_t* path) {
  char why[160] = "";
  const int rc = host_decode_rows(stream, desc, table, inflated, pixels, status, path, why, sizeof(why));
  if (rc || *status) cgan_set_error("cgan_png_decode_rows_host: %s", why);
  return rc ? CGAN_ERR_BAD_ARG : CGAN_OK;
}

extern "C" size_t cgan_png_decode_rows_workspace_bytes(const cgan_png_desc* descs_host, const uint32_t* tables_host, size_t table_len,
                                                       int32_t n) {
  uint32_t max_rows, cap;
  if (rows_ok("cgan_png_decode_rows_workspace_bytes", descs_host, tables_host, table_len, n, ~(size_t)0, false, 0, &max_rows, &cap))
    return 0;
  return carve(nullptr, descs_host, n, true).bytes;
}

extern "C" int cgan_png_decode_rows(const uint8_t* blob, size_t blob_bytes, const cgan_png_desc* descs_host,
                                    const cgan_png_desc* descs_dev, const uint32_t* tables_host, const uint32_t* tables_dev,
                                    size_t table_len, int32_t n, uint8_t* out, size_t out_bytes, int32_t* status, int32_t* path,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const RowPart rows{tables_host, tables_dev, table_len, path};
  return png_decode_impl("cgan_png_decode_rows", blob, blob_bytes, descs_host, descs_dev, &rows, n, out, out_bytes, status, workspace,
                         workspace_bytes, stream, (int32_t)SUBSEQ_BITS_DEFAULT, (int32_t)LANE_TOKENS_DEFAULT);
}
