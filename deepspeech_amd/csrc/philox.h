// Philox4x32-10 (Salmon et al., 2011), the counter-based generator of every stateless random
// draw on the device (specaug.hip, dropout.hip): one block of four 32-bit words from a counter of
// four words and a key of two. Integer arithmetic only, so ops/reference.py philox4x32 gives the
// same words bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace ds2 {

__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                              unsigned k1, unsigned (&x)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0, x[1] = c1, x[2] = c2, x[3] = c3;
}

}  // namespace ds2
