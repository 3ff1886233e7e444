// mfma_planes.hpp -- the device steps that the byte-plane kernels on v_mfma_i32_16x16x64_i8 share (fir_gen_kernels.hpp, cic2_kernels.hpp,
// fir_up_kernels.hpp): splitting samples into byte planes, loading an A fragment, recombining the plane accumulators and
// passing a step's 256 outputs through the XOR-swizzled LDS tile.  One definition per step; a step that differs between two kernels stays
// in those kernels, and so does a step whose helper call changes a kernel's compiled code (the helpers form their addresses AFTER their
// data for that reason: the instruction order of the caller's own text).  Device helpers only: no kernel and no host state lives here.
#pragma once
#include <cstddef>
#include <cstdint>

namespace acdsp {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef unsigned v2u __attribute__((ext_vector_type(2)));
typedef long v2l __attribute__((ext_vector_type(2)));

// gather byte `p` (0..3 of a dword) of four dwords into one dword
__device__ __forceinline__ unsigned gather4(unsigned d0, unsigned d1, unsigned d2, unsigned d3, int p) {
  const unsigned sel = 0x0c0c0400u + 0x0101u * (unsigned)p;               // result bytes: [d0.p, d1.p, 0, 0]
  const unsigned lo = __builtin_amdgcn_perm(d1, d0, sel);
  const unsigned hi = __builtin_amdgcn_perm(d3, d2, sel);
  return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}

// Byte plane pp of one 16-byte piece (16 / S samples; S = 2, anything else is taken as 4) -> 16 / S bytes at planes + pp * plane_bytes + off.  Every plane
// but the top one (PX - 1) holds unsigned bytes and is re-biased to signed; the kernels' corr undoes it.
template <int S, int PX>
__device__ __forceinline__ void put_piece_plane(const v4i &v, int pp, unsigned char *planes, int plane_bytes, int off) {
  if constexpr (S == 2) {
    const unsigned sel = pp == 0 ? 0x06040200u : 0x07050301u;   // byte pp of the four 16-bit samples in two dwords
    unsigned lo = __builtin_amdgcn_perm((unsigned)v.y, (unsigned)v.x, sel), hi = __builtin_amdgcn_perm((unsigned)v.w, (unsigned)v.z, sel);
    if (pp < PX - 1) { lo ^= 0x80808080u; hi ^= 0x80808080u; }
    *(v2u *)(planes + pp * plane_bytes + off) = (v2u){lo, hi};
  } else {
    unsigned w = gather4((unsigned)v.x, (unsigned)v.y, (unsigned)v.z, (unsigned)v.w, pp);
    if (pp < PX - 1) { w ^= 0x80808080u; }
    *(unsigned *)(planes + pp * plane_bytes + off) = w;
  }
}
// ... at a pointer the caller has formed
template <int S, int PX>
__device__ __forceinline__ void put_piece_plane(const v4i &v, int pp, unsigned char *dst) { put_piece_plane<S, PX>(v, pp, dst, 0, 0); }

// A fragment of this lane for (K block b, coefficient digit q) of a plan with nb blocks and pc digits: zero beyond them
__device__ __forceinline__ v4i a_frag(const v4i *__restrict__ frag, int nb, int pc, int b, int q, int lane) {
  return (b < nb && q < pc) ? frag[((size_t)q * nb + b) * 64 + lane] : (v4i){0, 0, 0, 0};
}

// y = corr + sum_w acc[w][r] 2^(8w)  (mod 2^64): element r of the NACC plane accumulators of equal weight
template <int NACC>
__device__ __forceinline__ uint64_t planes_to_u64(const v4i (&acc)[NACC], int r, int64_t corr) {
  uint64_t y = (uint64_t)corr;
#pragma unroll
  for (int w = 0; w < (NACC < 8 ? NACC : 8); w++) { y += (uint64_t)(int64_t)acc[w][r] << (8 * w); }
  return y;
}
// The 256 outputs of a step pass through an XOR-swizzled LDS tile into row order (conflict-free ds_write per column group and ds_read_b128
// per row run) and leave as whole 128-byte lines, 1 KB per instruction.  Lane (n_col, kg) puts its outputs 16 n_col + 4 kg + r, r = 0 .. 3,
// as OEB-byte containers.
template <int OEB, typename T>
__device__ __forceinline__ void tile_put(unsigned char *ob, int n_col, int kg, T o0, T o1, T o2, T o3) {
  if constexpr (OEB == 8) {
    const int L = 8 * n_col + 2 * kg, sw = n_col & 7;           // 16-byte slot of outputs r = 0, 1; r = 2, 3 follow
    *(v2l *)(ob + ((L ^ sw) * 16)) = (v2l){(long)o0, (long)o1};
    *(v2l *)(ob + (((L + 1) ^ sw) * 16)) = (v2l){(long)o2, (long)o3};
  } else if constexpr (OEB == 4) {
    const int L = 4 * n_col + kg;
    *(v4i *)(ob + ((L ^ ((n_col >> 1) & 3)) * 16)) = (v4i){(int)o0, (int)o1, (int)o2, (int)o3};
  } else {
    typedef short v4s_ __attribute__((ext_vector_type(4)));
    // unit 4 n_col + kg, low two bits XOR n_col >> 2: the 16 lanes of a ds_write_b64 bank pass (one kg) cover 16 distinct units mod 16
    *(v4s_ *)(ob + ((4 * n_col + kg) ^ ((n_col >> 2) & 3)) * 8) = (v4s_){(short)o0, (short)o1, (short)o2, (short)o3};
  }
}
// The wave reads the tile's row runs and stores its 256 OEB bytes (OEB = 8 or 4) at row + off; NT: non-temporal stores
template <int OEB, bool NT>
__device__ __forceinline__ void tile_flush(const unsigned char *ob, int lane, char *row, int64_t off) {
  static_assert(OEB == 8 || OEB == 4, "2-byte tiles leave in half-wave forms of their kernels");
  auto st = [](const v4i &val, v4i *ptr) {
    if constexpr (NT) { __builtin_nontemporal_store(val, ptr); } else { *ptr = val; }
  };
  if constexpr (OEB == 8) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int P = 64 * k + lane;
      const v4i val = *(const v4i *)(ob + ((P ^ ((P >> 3) & 7)) * 16));
      st(val, (v4i *)(row + off + 16 * P));
    }
  } else {
    const v4i val = *(const v4i *)(ob + ((lane ^ ((lane >> 3) & 3)) * 16));
    st(val, (v4i *)(row + off + 16 * lane));
  }
}

// Geometry of the LDS ring of byte planes (fir_gen_ring_kernel, cic2_kernel): S-byte samples, decimation R, NBT K blocks compiled in
template <int S, int R, int NBT>
struct RingGeom {
  static constexpr int LS = 8 / S;                                   // slots per 128-byte line
  static constexpr int ADV = 16 * R, NSL = 15 * R + 4 * NBT;         // slots a step advances / a step's window
  static constexpr int H = (LS - 1 + NSL - ADV + LS - 1) / LS * LS;  // halo slots (line multiple): covers any delta
  static constexpr int M = (R * S) % 4 == 0 ? 1 : 2;                 // steps per load group: a plain (R = 1) FIR on int16 advances half a 1 KB load per step, R = 5 two and a half
  static constexpr int NLD = R * S * M / 4;                          // 1 KB loads per group of M steps
  static constexpr int PPB = 16 / S;                                 // samples of a 16-byte piece = bytes of one of its planes
  static constexpr int SPK = 64 / S;                                 // slots per 1 KB load
};

}  // namespace acdsp
