// fir_long_kernels.hpp -- the segment geometry of the long int8-split Toeplitz kernels on the gfx950 matrix cores, shared by fir_long.hip
// (fir_long_kernel), polydec_long.hip (fir_long_dec_kernel) and polyintr_long.hip (fir_long_intr_kernel); fir_kernels.hpp stays the interface
// to the engine layer.
//
// The three kernels walk the K-blocks of a coefficient set in SEGMENTS of kLongSB = 16 blocks (fir_long.hip, header comment): the eight waves
// of a workgroup share one 32 KB A segment in LDS, double-buffered, and each wave stages its own sample window of the segment, 32 + 16 - 1 =
// 47 chunks, split into byte planes.  LDS: 2 x 32 KB + 8 waves x 2 x 4 x 832 B = 116 KB, one workgroup per CU, two waves per SIMD.
//
// The kernel bodies themselves are NOT shared.  One function template over a policy type (rows, window chunk, high-plane predicate,
// per-phase correction, final store) compiled to K-block loops of the same length but measured 0.4 - 1.8 % slower than the separate kernels
// on the short-nb shapes, outside the margin a refactor may cost (profiles/long_body_ab.txt); the three kernels keep their own text.
#pragma once

#include "fir_kernels.hpp"

namespace acdsp {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

constexpr int kLongSB = 16;                          // K-blocks per LDS segment
constexpr int kLongNC = 32 + kLongSB - 1;            // chunks (32 samples) of a segment's sample window
constexpr int kLongNP = 4 * kLongNC;                 // 16-byte loads of the window
constexpr int kLongJN = (kLongNP + 63) / 64;         // ... per lane
// one staged [plane][half] array of kLongNC 16-byte chunks (fir_mfma_kernels.hpp, staged_array_bytes: size = 64 mod 128 keeps the halves 16 banks apart)
constexpr int kLongARR = ((kLongNC * 16 + 63) / 128) * 128 + 64;
constexpr int kLongAWords = 2 * kLongSB * 64;        // v4i words of one A segment: [plane][block][lane]
constexpr int kLongAPerThread = kLongAWords / 512;   // = 4
constexpr int kLongXBytes = 4 * kLongARR;            // one staged window of a wave
constexpr size_t kLongLdsBytes = (size_t)2 * kLongAWords * 16 + (size_t)8 * 2 * kLongXBytes;
static_assert(kLongAWords % 512 == 0, "an A segment is copied by 512 threads in whole passes");
static_assert(kLongARR >= kLongNC * 16, "staged array holds the window");
static_assert(kLongLdsBytes <= 160 * 1024, "LDS of one gfx950 CU");

}  // namespace acdsp
