// The host entry points of the JPEG decoder without anything of HIP: jpeg_decode.hip wraps them into the C ABI
// (cgan_jpeg_parse_host, cgan_jpeg_decode_coefficients_host), tools/jpeg_decode_asan.cpp runs the same text under sanitizers.
// Each returns 0 or -1 (an argument refused, the reason in `why`); the file's status goes to *status.
#pragma once
#include <vector>

#include "jpeg_decode_core.h"

namespace jpeg_dec {

inline int host_parse(const uint8_t* file, size_t file_bytes, cgan_jpeg_desc* desc, int32_t* status, char* why, size_t why_len) {
  if (!file || !desc || !status) return snprintf(why, why_len, "null pointer"), -1;
  *status = parse(file, file_bytes, desc, why, why_len);
  return 0;
}

inline int host_subseq(int32_t subseq_bytes, uint32_t* subseq, char* why, size_t why_len) {
  if (subseq_bytes != 0 && (subseq_bytes < (int32_t)MIN_SUBSEQ || subseq_bytes > (int32_t)MAX_SUBSEQ))
    return snprintf(why, why_len, "subseq_bytes = %d: 0 (the default, %u) or %u .. %u", subseq_bytes, DEFAULT_SUBSEQ, MIN_SUBSEQ,
                    MAX_SUBSEQ), -1;
  *subseq = subseq_bytes ? (uint32_t)subseq_bytes : DEFAULT_SUBSEQ;
  return 0;
}

inline int host_decode_coefficients(const uint8_t* file, size_t file_bytes, const cgan_jpeg_desc* desc, int32_t subseq_bytes,
                                    int32_t round_cap, int16_t* coef, size_t coef_count, int32_t* rounds, int32_t* status,
                                    char* why, size_t why_len) {
  if (!file || !desc || !coef || !rounds || !status) return snprintf(why, why_len, "null pointer"), -1;
  uint32_t subseq;
  if (host_subseq(subseq_bytes, &subseq, why, why_len)) return -1;
  if (round_cap < 0) return snprintf(why, why_len, "round_cap = %d is negative", round_cap), -1;
  if (!desc_ok(*desc)) return snprintf(why, why_len, "not a descriptor the parser produces"), -1;
  if ((uint64_t)desc->scan_offset + desc->scan_bytes > file_bytes)
    return snprintf(why, why_len, "the scan reaches behind the file's end"), -1;
  const Frame f = frame(*desc);
  if (coef_count < 64 * (size_t)f.blocks)
    return snprintf(why, why_len, "coef holds %zu values, %lld are needed", coef_count, (long long)(64 * f.blocks)), -1;
  const uint32_t nchunks = chunks_of(desc->scan_bytes, subseq);
  std::vector<State> states(nchunks), entries(nchunks);
  std::vector<Count> counts(nchunks);
  memset(coef, 0, sizeof(int16_t) * 64 * (size_t)f.blocks);
  *status = (int32_t)decode_serial(*desc, file + desc->scan_offset, subseq, (uint32_t)round_cap, states.data(), entries.data(),
                                   counts.data(), coef, rounds);
  snprintf(why, why_len, "%s", *status == CGAN_JPEG_NOT_CONVERGED ? "the states did not converge" : (*status ? "corrupt data" : ""));
  return 0;
}

}  // namespace jpeg_dec
