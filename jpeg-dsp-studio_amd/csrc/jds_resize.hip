// jds_resize.hip — k_resize / k_resize_batch: packed RGB -> the bytes Pillow's
// Image.resize gives, both passes of an output tile in one workgroup (DESIGN.md
// "Pillow resizing").  The tile core is csrc/jds_resize.hpp, shared with the
// host tile loop (jds_selftest_resize) and tools/resize_san.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_internal.hpp"
#include "jds_resize.hpp"

namespace jds {

// The render kernels' budget of four workgroups per CU: 40 KB of LDS each at the
// most; three waves per workgroup leave the registers no constraint.
static_assert(sizeof(RsShared) <= 40 * 1024, "the LDS of four workgroups per CU");
#define RS_KERNEL __global__ void __launch_bounds__(RS_NT)

// One workgroup per tile, a lane per (column, channel).  r, tabs, tile and zero
// are uniform: the bounds and the vertical taps are read through them from the
// constant tables; the horizontal taps of the tile's columns go to LDS once.
__device__ __forceinline__ void rs_tile_dev(RsShared& sh, const RsRec& r, const int32_t* __restrict__ tabs,
                                            const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const int tile,
                                            const bool zero) {
  const int tid = threadIdx.x, c = tid / 3, ch = tid - 3 * c;
  const int ty = tile / r.tiles_x, tx = tile - ty * r.tiles_x;
  const RsTile t = rs_tile(r, tabs, ty, tx);
  const bool on = c < t.nc;
  int32_t acc[RS_TH];
#pragma unroll
  for (int i = 0; i < RS_TH; ++i) acc[i] = 0;
  if (!zero) {  // (uniform)
    if (r.needh)
      for (int e = tid; e < t.nc * r.ksh; e += RS_NT) sh.ht[e] = tabs[r.ht + (long long)t.X0 * r.ksh + e];
    int ya[RS_TH], yn[RS_TH];
    rs_windows(r, tabs, t, ya, yn);
    rs_acc_init(r, acc);
    RsCol k = {0, 0, 0};
    if (on) k = rs_col(r, tabs, t, c, ch);
    const int n = 3 * (t.xe - t.xs);
    const long long pitch = (long long)r.W * 3;
#pragma unroll 1
    for (int y = t.ys; y < t.ye; y += r.nr) {
      const int rows = t.ye - y < r.nr ? t.ye - y : r.nr;
      const uint8_t* g = src + ((long long)y * r.W + t.xs) * 3;
      __syncthreads();  // the taps are in place; the last step's rows have been read
      rs_stage_lane(sh.seg, r.segs, g, pitch, n, rows, tid, RS_NT);
      __syncthreads();
      if (on) {
#pragma unroll 1
        for (int q = 0; q < rows; ++q) {
          const uint8_t* row = sh.seg + q * r.segs + rs_phase(g + (long long)q * pitch);
          rs_vacc(r, tabs, t, ya, yn, y + q, rs_hsample(sh, row, k, r.needh != 0), acc);
        }
      }
    }
    rs_finish(r, acc);
  }
  __syncthreads();  // the staged rows become the output rows
  if (on) rs_emit(sh, r, t, dst, tid, acc);
  __syncthreads();
  rs_store_lane(sh.seg, RS_OS, rs_dst(r, t, dst), (long long)r.ow * 3, 3 * t.nc, t.nrw, tid, RS_NT);
}

RS_KERNEL
k_resize(const RsRec r, const int32_t* __restrict__ tabs, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst) {
  __shared__ RsShared sh;
  rs_tile_dev(sh, r, tabs, src + r.src_off, dst + r.dst_off, (int)blockIdx.x, r.zero != 0);
}

// A workgroup finds its record in the launch's map, as k_jpeg_ljs_batch does; a
// record whose status word is set, or that is flagged, gets zeros.  src1 / dst1:
// the scratch of the tall-image rule.
RS_KERNEL
k_resize_batch(const RsRec* __restrict__ recs, const RsMap* __restrict__ map, const int nmap,
               const uint32_t* __restrict__ status, const int32_t* __restrict__ tabs,
               const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1, uint8_t* __restrict__ dst0,
               uint8_t* __restrict__ dst1) {
  __shared__ RsShared sh;
  const int mi = rs_find(map, nmap, (int)blockIdx.x);
  const RsRec& r = recs[map[mi].rec];
  const int tile = (int)blockIdx.x - map[mi].tile0;
  const bool zero = r.zero != 0 || (r.st >= 0 && status[r.st] != 0u);
  rs_tile_dev(sh, r, tabs, (r.src_sel ? src1 : src0) + r.src_off, (r.dst_sel ? dst1 : dst0) + r.dst_off, tile, zero);
}

hipError_t launch_resize(const RsRec& r, const int32_t* tabs, const uint8_t* src, uint8_t* dst, hipStream_t s) {
  k_resize<<<dim3((unsigned)(r.tiles_y * r.tiles_x)), dim3(RS_NT), 0, s>>>(r, tabs, src, dst);
  kmark(s, "k_resize");
  return hipGetLastError();
}

hipError_t launch_resize_batch(const RsRec* recs, const RsMap* map, int nmap, int tiles, const uint32_t* status,
                               const int32_t* tabs, const uint8_t* src0, const uint8_t* src1, uint8_t* dst0,
                               uint8_t* dst1, hipStream_t s) {
  if (nmap < 1 || tiles < 1) return hipSuccess;
  k_resize_batch<<<dim3((unsigned)tiles), dim3(RS_NT), 0, s>>>(recs, map, nmap, status, tabs, src0, src1, dst0, dst1);
  kmark(s, "k_resize_batch");
  return hipGetLastError();
}

}  // namespace jds
