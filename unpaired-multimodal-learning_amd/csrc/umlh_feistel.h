// The epoch permutation pi_{n,seed} of 0..n-1, one definition for every kernel that needs an element of it: a 4-round Feistel
// network over 2*half bits keyed by `seed`, restricted to [0, n) by cycle walking (a bijection; O(1) per element, random access).
// feistel_perm_kernel writes the whole permutation, index_block_kernel only the slices a block of steps consumes.
#pragma once
#include <hip/hip_runtime.h>

// Half the bit width of the smallest even-width domain that holds n ids (n >= 1): the Feistel network permutes 2*half bits.
inline int feistel_half(long long n) {
    int bits = 1;
    while ((1LL << bits) < n) ++bits;
    return (bits + 1) / 2;
}

__device__ __forceinline__ unsigned mix32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}

// pi_{n,seed}(i) for 0 <= i < n; half = feistel_half(n)
__device__ __forceinline__ long long feistel_index(long long i, long long n, unsigned long long seed, int half) {
    const unsigned long long mask = (1ULL << half) - 1ULL;
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    unsigned long long x = (unsigned long long)i;
    do {
        unsigned long long L = x >> half, R = x & mask;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            unsigned long long F = (unsigned long long)mix32((unsigned)R * 0x9e3779b1U + (r & 1 ? k1 : k0) + 0x85ebca6bU * (unsigned)r +
                                                               (unsigned)(R >> 32)) & mask;
            unsigned long long nl = R;
            R = L ^ F;
            L = nl;
        }
        x = (L << half) | R;
    } while (x >= (unsigned long long)n);
    return (long long)x;
}
