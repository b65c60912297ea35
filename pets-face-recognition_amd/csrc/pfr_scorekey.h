// pfr_scorekey.h — the order-preserving uint32 of a score that the 64-bit "score, then smallest index" atomic-max keys carry
// (pfr_dbscan.hip: the border key; pfr_extremes.hip: best mate / best impostor / weakest mate): ONE definition of the map and its
// inverse, so that every key of the library has the same tie rule.
#pragma once
#include <hip/hip_runtime.h>

// score -> uint32 with the order of the floats (-0 canonicalised to +0 first; a NaN never gets here: it does not qualify)
__device__ __forceinline__ unsigned int db_score_key(float s) {
  const unsigned int u = __float_as_uint(s + 0.0f);
  return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u);
}

// the float whose db_score_key is k
__device__ __forceinline__ float db_key_score(unsigned int k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// (ord << 32) | (0xffffffff - partner): the maximum over keys is the highest ord, then the smallest partner
__device__ __forceinline__ unsigned long long db_pack_key(unsigned int ord, int partner) {
  return ((unsigned long long)ord << 32) | (unsigned long long)(0xffffffffu - (unsigned int)partner);
}
