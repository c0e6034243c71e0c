// JPEG decoder on the device: a batch of baseline files in one device blob -> one uint8 [h, w, c] image per file
// and one status word per file.  The parser (host), the per-subsequence decode step, the state, the table form, the status
// codes and the integer reconstruction are jpeg_decode_core.h: the kernels below call them, the host twin
// (cgan_jpeg_decode_coefficients_host) runs the same rounds serially.
//
// The scan of a file is cut into subsequences of `subseq` bytes, 256 of them are a tile = one workgroup.
//   layout_kernel   one thread: every file's places in the workspace (prefix sums over the files)
//   sync_kernel     min(SYNC_LAUNCHES, the most tiles a file has) times.  Thread t decodes subsequence t from the exit state of
//                   t - 1 and repeats while that state changes, behind __syncthreads(), until nothing changes in the tile (at
//                   most 257 rounds: after k
//                   rounds the tile's first k states follow from its entry state).  The tile's entry state is what the tile
//                   before it left in the PREVIOUS launch (tile_exit is double-buffered): no workgroup waits for another.
//                   From the second launch on a tile whose entry state did not change does nothing.
//   scan_kernel     one workgroup per file: exclusive segmented prefix sum over the subsequences of (markers crossed, blocks
//                   begun, DC differences per component) -> every subsequence's segment, write position and DC predictors
//   write_kernel    decodes every subsequence once more from its final entry state: the coefficients to their places (DC
//                   values, not differences), CORRUPT for what the core finds, NOT_CONVERGED if the exit state it gets is not
//                   the stored one (the stored states are then no fixpoint; if they are, they are exact by induction)
//   idct_kernel     one thread per block: dequantise, inverse DCT, samples into the component's plane
//   rgb_kernel      one thread per pixel: chroma upsampling, YCbCr -> RGB (or the grey plane copied)
// Launches and memsets per call: 2 memsets (status, coefficients) + layout + at most SYNC_LAUNCHES + scan + write + idct + rgb
// = at most 15.
//
// Bounds: the reader never touches a byte outside [scan, scan + scan_bytes) (Bits), a coefficient is written only to a block
// the frame has (WriteSink::place), every loop is bounded by the subsequence size, the tile size or the file count.
#include "cgan_common.h"
#include "jpeg_decode_host.h"

namespace {

using namespace jpeg_dec;

constexpr int T = 256;                 // threads per workgroup = subsequences per tile
// sync launches per call at most (fewer if no file has that many tiles): after k launches the first k tiles of a file are
// right by induction, so files of up to 8 tiles (256 KiB of scan at 128 bytes) always converge; longer ones do unless a
// decode that starts at a wrong place stays wrong for a whole tile, which the write pass reports as NOT_CONVERGED
constexpr int SYNC_LAUNCHES = 8;

struct FileLayout {
  int64_t block_off;                   // blocks of the files before this one: coefficients at 64 x, plane bytes at 64 x
  uint32_t chunk_off, tile_off, nchunks, ntiles;
};
struct Workspace {
  FileLayout* layout;
  State* state;
  State* entry_used;                   // per subsequence: the entry state its stored exit state was computed from
  Count* count;
  Count* before;
  State* tile_exit;                    // [2][tiles]
  int16_t* coef;
  uint8_t* planes;
  size_t bytes;
};
inline size_t align16(size_t v) { return (v + 15) / 16 * 16; }
// the same arithmetic for the size query and the call
Workspace carve(void* base, const cgan_jpeg_desc* descs, int32_t n, uint32_t subseq, uint32_t* max_tiles, int64_t* blocks,
                int64_t* max_blocks, int64_t* max_pixels) {
  uint64_t chunks = 0, tiles = 0;
  int64_t nb = 0, mb = 0, mp = 0;
  uint32_t mt = 0;
  for (int32_t i = 0; i < n; ++i) {
    const uint32_t c = chunks_of(descs[i].scan_bytes, subseq), t = (c + T - 1) / T;
    const Frame f = frame(descs[i]);
    chunks += c, tiles += t, nb += f.blocks;
    mt = t > mt ? t : mt, mb = f.blocks > mb ? f.blocks : mb;
    const int64_t px = (int64_t)descs[i].width * descs[i].height;
    mp = px > mp ? px : mp;
  }
  if (max_tiles) *max_tiles = mt;
  if (blocks) *blocks = nb;
  if (max_blocks) *max_blocks = mb;
  if (max_pixels) *max_pixels = mp;
  Workspace w;
  char* p = static_cast<char*>(base);
  size_t at = 0;
  auto take = [&](size_t bytes) {
    char* q = p + at;
    at += align16(bytes);
    return q;
  };
  w.layout = reinterpret_cast<FileLayout*>(take(sizeof(FileLayout) * (size_t)n));
  w.state = reinterpret_cast<State*>(take(sizeof(State) * chunks));
  w.entry_used = reinterpret_cast<State*>(take(sizeof(State) * chunks));
  w.count = reinterpret_cast<Count*>(take(sizeof(Count) * chunks));
  w.before = reinterpret_cast<Count*>(take(sizeof(Count) * chunks));
  w.tile_exit = reinterpret_cast<State*>(take(sizeof(State) * 2 * tiles));
  w.coef = reinterpret_cast<int16_t*>(take(sizeof(int16_t) * 64 * (size_t)nb));
  w.planes = reinterpret_cast<uint8_t*>(take(64 * (size_t)nb));
  w.bytes = at;
  return w;
}

__global__ void layout_kernel(const cgan_jpeg_desc* __restrict__ descs, int n, uint32_t subseq, FileLayout* __restrict__ layout) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  FileLayout at{0, 0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    at.nchunks = chunks_of(descs[i].scan_bytes, subseq);
    at.ntiles = (at.nchunks + T - 1) / T;
    layout[i] = at;
    at.block_off += frame(descs[i]).blocks;
    at.chunk_off += at.nchunks, at.tile_off += at.ntiles;
  }
}

// the file's six tables into LDS, once per workgroup
struct LdsTables {
  cgan_jpeg_hufftab dc[3], ac[3];
};
__device__ inline Tables stage_tables(LdsTables& lds, const cgan_jpeg_desc& d) {
  static_assert(sizeof(cgan_jpeg_hufftab) % 4 == 0 && sizeof(LdsTables) == 6 * sizeof(cgan_jpeg_hufftab), "copied as words");
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&d.dc[0]);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&lds);
  for (int k = threadIdx.x; k < (int)(sizeof(LdsTables) / 4); k += T) dst[k] = src[k];
  __syncthreads();
  return Tables{{&lds.dc[0], &lds.dc[1], &lds.dc[2]}, {&lds.ac[0], &lds.ac[1], &lds.ac[2]}};
}

__global__ __launch_bounds__(T) void sync_kernel(const uint8_t* __restrict__ blob, const cgan_jpeg_desc* __restrict__ descs,
                                                 uint32_t subseq, int launch, Workspace w, uint32_t tiles_total) {
  __shared__ LdsTables lds;
  __shared__ State sh[T];
  const int file = blockIdx.y, t = threadIdx.x;
  const FileLayout L = w.layout[file];
  if (blockIdx.x >= L.ntiles) return;
  const cgan_jpeg_desc& d = descs[file];
  const Tables tb = stage_tables(lds, d);
  const Frame f = frame(d);
  const uint8_t* scan = blob + d.blob_offset + d.scan_offset;
  const uint32_t len = d.scan_bytes;
  const uint32_t tile = blockIdx.x, chunk = tile * T + t;
  const bool live = chunk < L.nchunks;
  const size_t gi = (size_t)L.chunk_off + chunk;
  const State* exit_prev = w.tile_exit + (size_t)((launch + 1) & 1) * tiles_total + L.tile_off;
  State* exit_cur = w.tile_exit + (size_t)(launch & 1) * tiles_total + L.tile_off;

  State entry{0, 0};                          // of the tile: what thread 0 starts from
  if (tile > 0) entry = launch == 0 ? cold_state(scan, len, subseq, tile * T) : exit_prev[tile - 1];

  auto run = [&](State in) {
    CountSink sink;
    uint32_t err = 0;
    const State out = decode_chunk(tb, f, scan, len, subseq, chunk, L.nchunks, in, sink, err);
    w.count[gi] = sink.c;
    w.entry_used[gi] = in;
    return out;
  };
  State cur{0, 0}, used{0, 0};
  if (live) {
    if (launch == 0) {
      used = t == 0 ? entry : cold_state(scan, len, subseq, chunk);
      cur = run(used);
    } else {
      cur = w.state[gi], used = w.entry_used[gi];
    }
  }
  for (int round = 0; round <= T; ++round) {
    sh[t] = cur;
    __syncthreads();
    bool changed = false;
    if (live) {
      const State in = t == 0 ? entry : sh[t - 1];
      if (!same(in, used)) cur = run(in), used = in, changed = true;
    }
    if (!__syncthreads_or(changed)) break;
  }
  if (live) {
    w.state[gi] = cur;
    if (t == T - 1 || chunk + 1 == L.nchunks) exit_cur[tile] = cur;
  }
}

// one workgroup per file: thread t sums a run of consecutive subsequences, thread 0 scans the 256 sums, every thread walks its
// run again with its carry
__global__ __launch_bounds__(T) void scan_kernel(Workspace w) {
  __shared__ Count sums[T];
  const FileLayout L = w.layout[blockIdx.x];
  const int t = threadIdx.x;
  const uint32_t per = (L.nchunks + T - 1) / T;
  const uint32_t lo = (uint32_t)t * per < L.nchunks ? (uint32_t)t * per : L.nchunks;
  const uint32_t hi = lo + per < L.nchunks ? lo + per : L.nchunks;
  const Count* count = w.count + L.chunk_off;
  Count* before = w.before + L.chunk_off;
  Count acc{0, 0, {0, 0, 0}};
  for (uint32_t i = lo; i < hi; ++i) acc = combine(acc, count[i]);
  sums[t] = acc;
  __syncthreads();
  if (t == 0) {
    Count run{0, 0, {0, 0, 0}};
    for (int k = 0; k < T; ++k) {
      const Count mine = sums[k];
      sums[k] = run;
      run = combine(run, mine);
    }
  }
  __syncthreads();
  acc = sums[t];
  for (uint32_t i = lo; i < hi; ++i) {
    before[i] = acc;
    acc = combine(acc, count[i]);
  }
}

__global__ __launch_bounds__(T) void write_kernel(const uint8_t* __restrict__ blob, const cgan_jpeg_desc* __restrict__ descs,
                                                  uint32_t subseq, Workspace w, int16_t* __restrict__ coef_base,
                                                  int32_t* __restrict__ status) {
  __shared__ LdsTables lds;
  const int file = blockIdx.y;
  const FileLayout L = w.layout[file];
  if (blockIdx.x >= L.ntiles) return;
  const cgan_jpeg_desc& d = descs[file];
  const Tables tb = stage_tables(lds, d);
  const uint32_t chunk = blockIdx.x * T + threadIdx.x;
  if (chunk >= L.nchunks) return;
  const Frame f = frame(d);
  const size_t gi = (size_t)L.chunk_off + chunk;
  const State in = chunk == 0 ? State{0, 0} : w.state[gi - 1];
  uint32_t err = same(in, w.entry_used[gi]) ? 0u : (uint32_t)CGAN_JPEG_NOT_CONVERGED;
  WriteSink sink(f, coef_base + 64 * L.block_off, w.before[gi], in);
  const State out = decode_chunk(tb, f, blob + d.blob_offset + d.scan_offset, d.scan_bytes, subseq, chunk, L.nchunks, in, sink, err);
  if (!same(out, w.state[gi])) err |= CGAN_JPEG_NOT_CONVERGED;
  if (err) atomicOr(&status[file], (int32_t)err);
}

__global__ __launch_bounds__(T) void idct_kernel(const cgan_jpeg_desc* __restrict__ descs, Workspace w) {
  const int file = blockIdx.y;
  const cgan_jpeg_desc& d = descs[file];
  const Frame f = frame(d);
  const int64_t b = (int64_t)blockIdx.x * T + threadIdx.x;
  if (b >= f.blocks) return;
  const int64_t base = w.layout[file].block_off;
  const int comp = (f.ncomp == 3 && b >= f.off[1]) ? (b >= f.off[2] ? 2 : 1) : 0;
  const int64_t k = b - f.off[comp];
  const int by = (int)(k / f.bw[comp]), bx = (int)(k % f.bw[comp]);
  uint8_t px[64];
  idct_block(w.coef + 64 * (base + b), d.quant[comp], px);
  const int stride = 8 * f.bw[comp];
  uint8_t* dst = w.planes + 64 * (base + f.off[comp]) + ((int64_t)by * 8) * stride + bx * 8;
  for (int r = 0; r < 8; ++r) {
    u32x2 v;
    v.x = px[8 * r] | (px[8 * r + 1] << 8) | (px[8 * r + 2] << 16) | ((uint32_t)px[8 * r + 3] << 24);
    v.y = px[8 * r + 4] | (px[8 * r + 5] << 8) | (px[8 * r + 6] << 16) | ((uint32_t)px[8 * r + 7] << 24);
    *reinterpret_cast<u32x2*>(dst + (int64_t)r * stride) = v;           // 8-byte aligned: plane bases, strides and bx * 8 are
  }
}

__global__ __launch_bounds__(T) void rgb_kernel(const cgan_jpeg_desc* __restrict__ descs, Workspace w, uint8_t* __restrict__ out) {
  const int file = blockIdx.y;
  const cgan_jpeg_desc& d = descs[file];
  const int64_t p = (int64_t)blockIdx.x * T + threadIdx.x;
  if (p >= (int64_t)d.width * d.height) return;
  const Frame f = frame(d);
  const int y = (int)(p / d.width), x = (int)(p % d.width);
  const uint8_t* planes = w.planes + 64 * w.layout[file].block_off;
  const int luma = planes[(int64_t)y * (8 * f.bw[0]) + x];
  uint8_t* o = out + d.out_offset + p * d.ncomp;
  if (d.ncomp == 1) {
    o[0] = (uint8_t)luma;
    return;
  }
  const int cw = (d.width + d.hs - 1) / d.hs, ch = (d.height + d.vs - 1) / d.vs;
  const int cb = chroma_at(planes + 64 * f.off[1], 8 * f.bw[1], cw, ch, d.hs, d.vs, y, x);
  const int cr = chroma_at(planes + 64 * f.off[2], 8 * f.bw[2], cw, ch, d.hs, d.vs, y, x);
  ycc_to_rgb(luma, cb, cr, o);
}

int subseq_of(const char* what, int32_t subseq_bytes, uint32_t* subseq) {
  char why[160];
  CGAN_REQUIRE(host_subseq(subseq_bytes, subseq, why, sizeof(why)) == 0, "%s: %s", what, why);
  return CGAN_OK;
}

int descs_ok(const char* what, const cgan_jpeg_desc* descs, int32_t n, size_t blob_bytes, bool with_out, size_t out_bytes) {
  CGAN_REQUIRE(descs, "%s: null pointer", what);
  CGAN_REQUIRE(n >= 1 && n <= 65535, "%s: n = %d: 1 <= n <= 65535 expected", what, n);
  for (int32_t i = 0; i < n; ++i) {
    const cgan_jpeg_desc& d = descs[i];
    CGAN_REQUIRE(desc_ok(d), "%s: descriptor %d is not one the parser produces", what, i);
    CGAN_REQUIRE(d.blob_offset >= 0 && (uint64_t)d.blob_offset + d.scan_offset + d.scan_bytes <= blob_bytes,
                 "%s: the scan of file %d reaches behind the blob's end", what, i);
    if (with_out)
      CGAN_REQUIRE(d.out_offset >= 0 && (uint64_t)d.out_offset + (uint64_t)d.width * d.height * d.ncomp <= out_bytes,
                   "%s: the pixels of file %d reach behind the output's end", what, i);
  }
  return CGAN_OK;
}

int decode(const char* what, const uint8_t* blob, size_t blob_bytes, const cgan_jpeg_desc* descs_host,
           const cgan_jpeg_desc* descs_dev, int32_t n, int32_t subseq_bytes, uint8_t* out, size_t out_bytes, int16_t* coef_out,
           size_t coef_count, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  CGAN_REQUIRE(blob && descs_dev && status && workspace && (out || coef_out), "%s: null pointer", what);
  uint32_t subseq;
  if (const int rc = subseq_of(what, subseq_bytes, &subseq)) return rc;
  if (const int rc = descs_ok(what, descs_host, n, blob_bytes, out != nullptr, out_bytes)) return rc;
  CGAN_REQUIRE(reinterpret_cast<uintptr_t>(workspace) % 16 == 0, "%s: the workspace is not 16-byte aligned", what);
  uint32_t max_tiles;
  int64_t blocks, max_blocks, max_pixels;
  const Workspace w0 = carve(workspace, descs_host, n, subseq, &max_tiles, &blocks, &max_blocks, &max_pixels);
  if (w0.bytes > workspace_bytes) {
    cgan_set_error("%s: the workspace has %zu bytes, %zu are needed", what, workspace_bytes, w0.bytes);
    return CGAN_ERR_WORKSPACE;
  }
  Workspace w = w0;
  if (coef_out) {
    CGAN_REQUIRE(coef_count >= 64 * (size_t)blocks, "%s: coef holds %zu values, %lld are needed", what, coef_count,
                 (long long)(64 * blocks));
    w.coef = coef_out;
  }
  uint64_t tiles_total = 0;
  for (int32_t i = 0; i < n; ++i) tiles_total += (chunks_of(descs_host[i].scan_bytes, subseq) + T - 1) / T;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (hipMemsetAsync(status, 0, sizeof(int32_t) * (size_t)n, s) != hipSuccess ||
      hipMemsetAsync(w.coef, 0, sizeof(int16_t) * 64 * (size_t)blocks, s) != hipSuccess) {
    cgan_set_error("%s: hipMemsetAsync failed", what);
    return CGAN_ERR_HIP;
  }
  hipLaunchKernelGGL(layout_kernel, dim3(1), dim3(64), 0, s, descs_dev, n, subseq, w.layout);
  CGAN_CHECK_LAUNCH("cgan_jpeg_decode (layout)");
  for (int k = 0; k < SYNC_LAUNCHES && (k == 0 || (uint32_t)k < max_tiles); ++k) {
    hipLaunchKernelGGL(sync_kernel, dim3(max_tiles, n), dim3(T), 0, s, blob, descs_dev, subseq, k, w, (uint32_t)tiles_total);
    CGAN_CHECK_LAUNCH("cgan_jpeg_decode (sync)");
  }
  hipLaunchKernelGGL(scan_kernel, dim3(n), dim3(T), 0, s, w);
  CGAN_CHECK_LAUNCH("cgan_jpeg_decode (scan)");
  hipLaunchKernelGGL(write_kernel, dim3(max_tiles, n), dim3(T), 0, s, blob, descs_dev, subseq, w, w.coef, status);
  CGAN_CHECK_LAUNCH("cgan_jpeg_decode (write)");
  if (!out) return CGAN_OK;
  hipLaunchKernelGGL(idct_kernel, dim3((unsigned)((max_blocks + T - 1) / T), n), dim3(T), 0, s, descs_dev, w);
  CGAN_CHECK_LAUNCH("cgan_jpeg_decode (idct)");
  hipLaunchKernelGGL(rgb_kernel, dim3((unsigned)((max_pixels + T - 1) / T), n), dim3(T), 0, s, descs_dev, w, out);
  CGAN_CHECK_LAUNCH("cgan_jpeg_decode (rgb)");
  return CGAN_OK;
}

}  // namespace

extern "C" int cgan_jpeg_parse_host(const uint8_t* file, size_t file_bytes, cgan_jpeg_desc* desc, int32_t* status) {
  char why[160] = "";
  const int rc = host_parse(file, file_bytes, desc, status, why, sizeof(why));
  if (rc || *status) cgan_set_error("cgan_jpeg_parse_host: %s", why);
  return rc ? CGAN_ERR_BAD_ARG : CGAN_OK;
}

extern "C" int cgan_jpeg_decode_coefficients_host(const uint8_t* file, size_t file_bytes, const cgan_jpeg_desc* desc,
                                                  int32_t subseq_bytes, int32_t round_cap, int16_t* coef, size_t coef_count,
                                                  int32_t* rounds, int32_t* status) {
  char why[160] = "";
  const int rc = host_decode_coefficients(file, file_bytes, desc, subseq_bytes, round_cap, coef, coef_count, rounds, status, why,
                                          sizeof(why));
  if (rc || *status) cgan_set_error("cgan_jpeg_decode_coefficients_host: %s", why);
  return rc ? CGAN_ERR_BAD_ARG : CGAN_OK;
}

extern "C" size_t cgan_jpeg_decode_workspace_bytes(const cgan_jpeg_desc* descs_host, int32_t n, int32_t subseq_bytes) {
  uint32_t subseq;
  if (subseq_of("cgan_jpeg_decode_workspace_bytes", subseq_bytes, &subseq)) return 0;
  if (descs_ok("cgan_jpeg_decode_workspace_bytes", descs_host, n, ~(size_t)0, false, 0)) return 0;
  return carve(nullptr, descs_host, n, subseq, nullptr, nullptr, nullptr, nullptr).bytes;
}

extern "C" int cgan_jpeg_decode_u8(const uint8_t* blob, size_t blob_bytes, const cgan_jpeg_desc* descs_host,
                                   const cgan_jpeg_desc* descs_dev, int32_t n, int32_t subseq_bytes, uint8_t* out,
                                   size_t out_bytes, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
  CGAN_REQUIRE(out, "cgan_jpeg_decode_u8: null pointer");
  return decode("cgan_jpeg_decode_u8", blob, blob_bytes, descs_host, descs_dev, n, subseq_bytes, out, out_bytes, nullptr, 0,
                status, workspace, workspace_bytes, stream);
}

extern "C" int cgan_jpeg_decode_coefficients(const uint8_t* blob, size_t blob_bytes, const cgan_jpeg_desc* descs_host,
                                             const cgan_jpeg_desc* descs_dev, int32_t n, int32_t subseq_bytes, int16_t* coef,
                                             size_t coef_count, int32_t* status, void* workspace, size_t workspace_bytes,
                                             void* stream) {
  CGAN_REQUIRE(coef, "cgan_jpeg_decode_coefficients: null pointer");
  return decode("cgan_jpeg_decode_coefficients", blob, blob_bytes, descs_host, descs_dev, n, subseq_bytes, nullptr, 0, coef,
                coef_count, status, workspace, workspace_bytes, stream);
}
