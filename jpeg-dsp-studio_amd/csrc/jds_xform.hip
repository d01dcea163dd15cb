// jds_xform.hip — k_coef_xform: the coefficient side of the lossless
// transforms (DESIGN.md "Lossless transforms"; definition:
// tests/transform_ref.py).  Between the batch decode and the writer's first
// kernel it rewrites the decoder's planes of every transformed file of a batch
// into the transformed geometry: a block permutation, an in-block transpose
// and / or sign flips.  The writer then reads the destination planes through
// its own McuFile; no k_mcu_* kernel knows about it.
//   * work is indexed by DESTINATION block: a tile (workgroup of 256) is
//     XF_BLOCKS = 32 consecutive blocks of one component's destination grid of
//     one file, a lane owns one row of one block: 8 coefficients, one 16-byte
//     store, a wave's stores cover 1 KiB of consecutive addresses;
//   * without XF_T the lane's source is one 16-byte load of the same row of
//     the source block (xf_src_block); the signs are a lane-uniform row parity
//     (XF_FV) and a constant mask over the odd columns (XF_FH);
//   * with XF_T the source block is staged through LDS: each lane stores its
//     16-byte source row, then gathers its destination row as one column with
//     eight 2-byte reads.  A block's 128 bytes sit 144 bytes apart (36 dwords),
//     so the four blocks of a 32-lane group read banks 36 b + 4 u + [0, 4) mod
//     32 = four disjoint runs of four banks: no conflict (two lanes that share
//     a dword read the same address);
//   * a negation is done in 32 bits and the low half stored, so -32768 stays
//     -32768 as in NumPy's int16 arithmetic;
//   * no scratch memory, no atomics, plain vector stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_internal.hpp"
#include "jds_xform.hpp"
#include "jds_xform_dev.hpp"

namespace jds {

constexpr int XF_LDS_ROW = 9;  // uint4 per staged block: 128 bytes of coefficients, 16 of padding

__global__ void __launch_bounds__(8 * XF_BLOCKS) k_coef_xform(const XfFile* __restrict__ files,
                                                              const int32_t* __restrict__ tilefile,
                                                              const int16_t* src, int16_t* dst) {
  __shared__ uint4 stage[XF_BLOCKS][XF_LDS_ROW];
  const int tile = blockIdx.x;
  const XfFile& F = files[__builtin_amdgcn_readfirstlane(tilefile[tile])];
  const int lt = tile - F.tile0;
  // (selects, not F.dgw[c]: the record's fields are scalar loads)
  const int c = lt >= F.ctile[2] ? 2 : (lt >= F.ctile[1] ? 1 : 0);
  const int ct = c == 0 ? F.ctile[0] : (c == 1 ? F.ctile[1] : F.ctile[2]);
  const int dgw = c == 0 ? F.dgw[0] : (c == 1 ? F.dgw[1] : F.dgw[2]);
  const int dgh = c == 0 ? F.dgh[0] : (c == 1 ? F.dgh[1] : F.dgh[2]);
  const int sgw = c == 0 ? F.sgw[0] : (c == 1 ? F.sgw[1] : F.sgw[2]);
  const long long soff = c == 0 ? F.soff[0] : (c == 1 ? F.soff[1] : F.soff[2]);
  const long long doff = c == 0 ? F.doff[0] : (c == 1 ? F.doff[1] : F.doff[2]);
  const int flags = F.flags;
  const int lb = threadIdx.x >> 3, v = threadIdx.x & 7;
  const int b = (lt - ct) * XF_BLOCKS + lb;  // the destination block in its grid's raster order
  const bool live = b < dgw * dgh;
  uint4 w = make_uint4(0u, 0u, 0u, 0u);
  if (live) {
    const int r = b / dgw, q = b - r * dgw;
    const long long a = xf_src_block(flags, dgw, dgh, sgw, soff, r, q);
    w = *reinterpret_cast<const uint4*>(src + a + 8 * v);
  }
  if (flags & XF_T) {  // (uniform over the workgroup)
    stage[lb][v] = w;
    __syncthreads();
    const uint16_t* col = reinterpret_cast<const uint16_t*>(&stage[lb][0]) + v;
    uint32_t x[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) x[u] = col[8 * u];
    w = make_uint4(x[0] | (x[1] << 16), x[2] | (x[3] << 16), x[4] | (x[5] << 16), x[6] | (x[7] << 16));
  }
  if (!live) return;
  // destination row v: every entry with XF_FV on an odd row, the odd columns with XF_FH
  const bool nv = (flags & XF_FV) && (v & 1), nh = (flags & XF_FH) != 0;
  const bool neg_even = nv, neg_odd = nv != nh;
  uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    uint32_t lo = d[i] & 0xFFFFu, hi = d[i] >> 16;
    lo = neg_even ? (0u - lo) & 0xFFFFu : lo;  // (two's complement: the low half of the 32-bit negation)
    hi = neg_odd ? (0u - hi) & 0xFFFFu : hi;
    d[i] = lo | (hi << 16);
  }
  *reinterpret_cast<uint4*>(dst + doff + 64ll * b + 8 * v) = make_uint4(d[0], d[1], d[2], d[3]);
}

hipError_t launch_coef_xform(const XfFile* files, const int32_t* tilefile, long long ntiles, const int16_t* src,
                             int16_t* dst, hipStream_t s) {
  if (ntiles <= 0) return hipSuccess;
  if (ntiles > 0x7fffffffll) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_coef_xform, dim3((unsigned)ntiles), dim3(8 * XF_BLOCKS), 0, s, files, tilefile, src, dst);
  kmark(s, "k_coef_xform");
  return hipGetLastError();
}

}  // namespace jds
