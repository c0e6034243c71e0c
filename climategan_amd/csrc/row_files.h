// Files assembled from independently coded rows: what the PNG and the JPEG encoder share.  A rows kernel codes
// every row into its staging slot and notes its size; a finish kernel, one workgroup per image, scans the sizes into
// offsets (row_offsets) and writes what stands around the rows; a gather kernel, one workgroup per row, moves the slots
// into the file (copy_row).  The workspace holds tables of one uint32 per row and, behind them, the slots.
#pragma once
#include "cgan_common.h"

namespace row_files {

constexpr int T = 256;                      // threads per workgroup, every kernel of both encoders
constexpr int MAX_W = 4096;                 // widest image, pixels (PNG: 12 288 filtered bytes as RGB, its LDS limit)

// inclusive scan of s[0 .. T) in place; the caller has written s[threadIdx.x] and passed a barrier.  Every s[] is final and
// readable by every thread on return.
__device__ inline void scan(uint32_t* s) {
  const int t = threadIdx.x;
  for (int k = 1; k < T; k <<= 1) {
    const uint32_t x = t >= k ? s[t - k] : 0u;
    __syncthreads();
    s[t] += x;
    __syncthreads();
  }
}

// One image's row offsets: the exclusive scan of its rows' sizes from `first`, T rows at a time, `gap` bytes behind every
// row but the last.  -> the offset behind the last row.  scratch: T words of LDS.
__device__ inline uint32_t row_offsets(uint32_t* scratch, const uint32_t* row_size, uint32_t* row_off, int rows, uint32_t first,
                                       uint32_t gap) {
  const int t = threadIdx.x;
  uint32_t running = first;
  for (int r0 = 0; r0 < rows; r0 += T) {
    const int r = r0 + t;
    const uint32_t v = r < rows ? row_size[r] + (r + 1 < rows ? gap : 0u) : 0u;
    scratch[t] = v;
    __syncthreads();
    scan(scratch);
    if (r < rows) row_off[r] = running + scratch[t] - v;
    running += scratch[T - 1];
    __syncthreads();
  }
  return running;
}

// A row's `size` bytes from `skip` bytes into its slot to dst, by the whole workgroup -> behind the copied bytes.  The row
// starts at any byte offset of the file, so it moves byte by byte.
__device__ inline uint8_t* copy_row(const uint8_t* slot, uint32_t skip, uint32_t size, uint8_t* dst) {
  for (uint32_t k = threadIdx.x; k < size; k += T) dst[k] = slot[skip + k];
  return dst + size;
}

// ---- the workspace: tables of one uint32 per row, each padded to 16 bytes; table(ws, rows, number of tables) = the slots
inline size_t table_bytes(int64_t rows) { return (size_t)((rows * 4 + 15) / 16 * 16); }
inline uint32_t* table(void* workspace, int64_t rows, int k) {
  return reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(workspace) + (size_t)k * table_bytes(rows));
}

// ---- refusals, with the caller's name ----------------------------------------------------------------------------------
inline bool channels_ok(const char* what, int32_t c) {
  if (c != 1 && c != 3) cgan_set_error("%s: c = %d: 8-bit grey (1) or RGB (3) only", what, c);
  return c == 1 || c == 3;
}
// n images of `rows` rows each: one workgroup per (row, image), grid.y = n
inline bool grid_ok(int64_t n, int64_t rows) { return n >= 1 && n <= 65535 && rows >= 1 && n * rows <= 0x7fffffffll; }
inline bool file_fits(const char* what, int32_t h, int32_t w, int32_t c, uint64_t bound) {
  if (bound > 0x7fffffffull)
    cgan_set_error("%s: a %d x %d x %d image may need %llu bytes, more than the 2^31 - 1 one file may have", what, h, w, c,
                   (unsigned long long)bound);
  return bound <= 0x7fffffffull;
}
// the output's pitch against the file's bound, the workspace against its size -> CGAN_OK or the error
inline int buffers_ok(const char* what, size_t out_pitch, size_t bound, const void* workspace, size_t workspace_bytes,
                      size_t need) {
  CGAN_REQUIRE(out_pitch >= bound, "%s: out_pitch %zu is below the bound %zu", what, out_pitch, bound);
  if (workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 15u)) {
    cgan_set_error("%s: workspace of %zu bytes (16-byte aligned) expected, got %zu at %p", what, need, workspace_bytes,
                   workspace);
    return CGAN_ERR_WORKSPACE;
  }
  return CGAN_OK;
}

}  // namespace row_files
