// jds_jpeg_ljs.hip — k_jpeg_ljs<SS, DENOM>: decoded coefficients of a baseline
// JPEG -> the RGB bytes libjpeg gives at scale 1/2, 1/4 or 1/8, in one launch
// (DESIGN.md "Scaled libjpeg rendering").  The tile core is
// csrc/jds_jpeg_ljs.hpp, shared with the host tile loop
// (jds_selftest_jpeg_render_scaled) and tools/jpeg_ljs_san.cpp; arguments,
// records and maps are k_jpeg_inv's, the tile grid is k_jpeg_ljt's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_internal.hpp"
#include "jds_jpeg_ljs.hpp"

namespace jds {

// k_jpeg_ljt's budget: four workgroups of 512 lanes per CU, so at most 40 KB of
// LDS and 64 VGPRs.  The largest LsShared is 4:2:0 at 1/2: 18 KB transpose
// buffer + 4.25 KB window + 3 KB staging + tables.
static_assert(sizeof(LsShared<JDS_SS_420, 2>) <= 40 * 1024 && sizeof(LsShared<JDS_SS_422, 2>) <= 40 * 1024 &&
                  sizeof(LsShared<JDS_SS_444, 2>) <= 40 * 1024 && sizeof(LsShared<JDS_SS_GRAY, 2>) <= 40 * 1024,
              "the LDS of four workgroups per CU");
#define LS_KERNEL __global__ void __launch_bounds__(JI_NT) __attribute__((amdgpu_waves_per_eu(8, 8)))

// One workgroup per tile, eight lanes per block.  A block's two passes run on 8
// lanes of one wave, whose LDS operations execute in order: wave barriers
// between them; workgroup barriers once the chroma window is complete and once
// the staging tile is.  a: uniform (the kernel argument or the image's record).
template <int SS, int D>
__device__ __forceinline__ void ls_tile_dev(LsShared<SS, D>& sh, const JInvArgs& a, const int tile,
                                            const int16_t* __restrict__ coeffs, uint8_t* __restrict__ rgb) {
  using C = LsCfg<SS, D>;
  const int tid = threadIdx.x, v = tid & 7, lb = tid >> 3;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const LsGeo g = ls_geo<SS, D>(a);
  const JWin w = ls_tile_window<SS, D>(g, ty, tx);
  if (tid < (SS == JDS_SS_GRAY ? 64 : 192)) sh.q[tid] = a.q[tid >> 6][tid & 63];
  __syncthreads();
  if constexpr (C::WIN) {
    const int ntask = 2 * w.ncbr * w.ncbc;
#pragma unroll 1
    for (int t = lb; t < ntask; t += JI_NB) {
      ls_chroma_col<SS, D>(sh, a, w, coeffs, t, v);
      __builtin_amdgcn_wave_barrier();
      ls_chroma_row<SS, D>(sh, a, g, w, t, v);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
  int by, bx;
  if (ls_luma_block(a, ty, tx, lb, &by, &bx)) {
    int32_t* mid = sh.mid + lb * LJ_MS;
    const long long boff = ((long long)by * a.gc[0] + bx) * 64;
    const int y = by * C::M + v, x0 = bx * C::M;
    const bool rowlane = v < C::M;
    int Yv[C::M] = {}, Cb[C::M] = {}, Cr[C::M] = {};
    ls_col<C::M>(coeffs + a.off[0] + boff, sh.q, v, mid);
    __builtin_amdgcn_wave_barrier();
    if (rowlane) ls_row<C::M>(mid, v, Yv);
    if constexpr (SS == JDS_SS_444) {  // the co-sited chroma blocks through the same slot
      __builtin_amdgcn_wave_barrier();
      ls_col<C::M>(coeffs + a.off[1] + boff, sh.q + 64, v, mid);
      __builtin_amdgcn_wave_barrier();
      if (rowlane) ls_row<C::M>(mid, v, Cb);
      __builtin_amdgcn_wave_barrier();
      ls_col<C::M>(coeffs + a.off[2] + boff, sh.q + 128, v, mid);
      __builtin_amdgcn_wave_barrier();
      if (rowlane) ls_row<C::M>(mid, v, Cr);
    }
    if (rowlane && y <= w.y1) {
      if constexpr (C::WIN) {
        ls_chroma_px<SS, D>(sh, g, w, y, x0, 0, Cb);
        ls_chroma_px<SS, D>(sh, g, w, y, x0, 1, Cr);
      }
      ls_emit<SS, D>(sh, w, y, x0, Yv, Cb, Cr);
    }
  }
  __syncthreads();
  ls_store<SS, D>(sh, g, w, rgb, tid);
}

template <int SS, int D>
LS_KERNEL
k_jpeg_ljs(const JInvArgs a, const int16_t* __restrict__ coeffs, uint8_t* __restrict__ rgb) {
  __shared__ LsShared<SS, D> sh;
  ls_tile_dev<SS, D>(sh, a, blockIdx.x, coeffs, rgb);
}

// k_jpeg_ljt_batch's contract: a workgroup finds its image in the launch's map;
// an image whose status word is set gets zeros; nothing between images is written.
template <int SS, int D>
LS_KERNEL
k_jpeg_ljs_batch(const JInvRec* __restrict__ recs, const JInvMap* __restrict__ map, const int nmap,
                 const uint32_t* __restrict__ status, const int16_t* __restrict__ coeffs,
                 uint8_t* __restrict__ rgb) {
  using C = LsCfg<SS, D>;
  __shared__ LsShared<SS, D> sh;
  const int mi = jinv_find(map, nmap, (int)blockIdx.x);
  const JInvRec& r = recs[map[mi].rec];
  const int tile = (int)blockIdx.x - map[mi].tile0;
  uint8_t* o = rgb + r.rgb_off;
  if (status[r.st] != 0u) {  // (uniform)
    const JInvArgs& a = r.a;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const LsGeo g = ls_geo<SS, D>(a);
    const JWin w = ls_tile_window<SS, D>(g, ty, tx);
    for (int i = threadIdx.x; i < 3 * C::TH * C::TW; i += JI_NT) ls_zero_lane(g, w, o, i);
    return;
  }
  ls_tile_dev<SS, D>(sh, r.a, tile, coeffs + r.coef_off, o);
}

// One launch on s; nothing is uploaded or read back.  denom: 2, 4 or 8.
hipError_t launch_jpeg_ljs(const JInvArgs& a, int denom, const int16_t* coeffs, uint8_t* rgb, hipStream_t s) {
  const dim3 grid((unsigned)(a.tiles_y * a.tiles_x)), block(JI_NT);
#define LS_CALL_(SS, D) k_jpeg_ljs<SS, D><<<grid, block, 0, s>>>(a, coeffs, rgb)
  LS_DISPATCH(a.ss, denom, LS_CALL_);
#undef LS_CALL_
  kmark(s, "k_jpeg_ljs<%d,%d>", a.ss, denom);
  return hipGetLastError();
}

// The scaled images of a batch: one launch per (mode, denominator) present.
// map_off / nmap / tiles: per mode and denominator index (2, 4, 8).
hipError_t launch_jpeg_ljs_batch(const JInvRec* recs, const JInvMap* maps, const int map_off[JI_MODES][LS_ND],
                                 const int nmap[JI_MODES][LS_ND], const int tiles[JI_MODES][LS_ND],
                                 const uint32_t* status, const int16_t* coeffs, uint8_t* rgb, hipStream_t s) {
  const dim3 block(JI_NT);
  for (int m = 0; m < JI_MODES; ++m)
    for (int d = 0; d < LS_ND; ++d) {
      if (nmap[m][d] < 1) continue;
      const dim3 grid((unsigned)tiles[m][d]);
      const JInvMap* mp = maps + map_off[m][d];
#define LS_CALL_(SS, D) k_jpeg_ljs_batch<SS, D><<<grid, block, 0, s>>>(recs, mp, nmap[m][d], status, coeffs, rgb)
      LS_DISPATCH(m, 2 << d, LS_CALL_);
#undef LS_CALL_
      kmark(s, "k_jpeg_ljs_batch<%d,%d>", m, 2 << d);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

}  // namespace jds
