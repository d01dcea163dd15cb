// jds_jpeg_ljt.hip — k_jpeg_ljt: decoded coefficients of a baseline JPEG -> the
// RGB bytes libjpeg's default decode gives, in one launch (DESIGN.md "libjpeg
// rendering").  The tile core is csrc/jds_jpeg_ljt.hpp, shared with the host
// tile loop (jds_selftest_jpeg_render) and tools/jpeg_ljt_san.cpp; arguments,
// tile, records and maps are k_jpeg_inv's (csrc/jds_jpeg_inv.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_internal.hpp"
#include "jds_jpeg_ljt.hpp"

namespace jds {

// 18 KB transpose buffer + tables; 4:2:0: + 6.8 KB window, 4:2:2: + 12 KB: the
// LDS of four workgroups of 512 lanes (all 32 wave slots of a CU) is within the
// 160 KB.  Registers: a workgroup is two waves per SIMD, so four need 8 waves
// per SIMD, i.e. at most 64 VGPRs and 80 SGPRs.  Left alone the compiler takes
// 106 SGPRs for the 4:2:0 instantiations (6 waves per SIMD, three workgroups);
// LJ_KERNEL asks for 8, which it meets with 78 SGPRs by keeping 25 (batch: 34)
// scalars in VGPR lanes -- VGPRs stay at 56 / 54, no scratch.  The other
// instantiations are below both limits either way.
static_assert(sizeof(LjShared<JDS_SS_422>) <= 40 * 1024 && sizeof(LjShared<JDS_SS_420>) <= 40 * 1024 &&
                  sizeof(LjShared<JDS_SS_444>) <= 40 * 1024 && sizeof(LjShared<JDS_SS_GRAY>) <= 40 * 1024,
              "the LDS of four workgroups per CU");
#define LJ_KERNEL __global__ void __launch_bounds__(JI_NT) __attribute__((amdgpu_waves_per_eu(8, 8)))

// One workgroup per tile, eight lanes per block (lane v: column v, then row v).
// A block's two passes run on 8 lanes of one wave, whose LDS operations execute
// in order: wave barriers between them, a workgroup barrier only once the chroma
// window is complete.  a: uniform (the kernel argument or the image's record).
template <int SS>
__device__ __forceinline__ void lj_tile_dev(LjShared<SS>& sh, const JInvArgs& a, const int tile,
                                            const int16_t* __restrict__ coeffs, uint8_t* __restrict__ rgb) {
  using C = LjCfg<SS>;
  const int tid = threadIdx.x, v = tid & 7, lb = tid >> 3;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const JWin w = lj_tile_window<SS>(a, ty, tx);
  if (tid < (SS == JDS_SS_GRAY ? 64 : 192)) sh.q[tid] = a.q[tid >> 6][tid & 63];
  __syncthreads();
  if constexpr (C::SX == 2) {
    const int ntask = 2 * w.ncbr * w.ncbc;
#pragma unroll 1
    for (int t = lb; t < ntask; t += JI_NB) {
      lj_chroma_col<SS>(sh, a, w, coeffs, t, v);
      __builtin_amdgcn_wave_barrier();
      lj_chroma_row<SS>(sh, a, w, t, v);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
  int by, bx;
  if (!jinv_luma_block(a, w, lb, &by, &bx)) return;  // (no barrier follows)
  int32_t* mid = sh.mid + lb * LJ_MS;
  const long long boff = ((long long)by * a.gc[0] + bx) * 64;
  const int y = by * 8 + v, x0 = bx * 8;
  int Yv[8], Cb[8], Cr[8];
  lj_col(coeffs + a.off[0] + boff, sh.q, v, mid);
  __builtin_amdgcn_wave_barrier();
  lj_row(mid, v, Yv);
  if constexpr (SS == JDS_SS_444) {  // the co-sited chroma blocks through the same slot
    __builtin_amdgcn_wave_barrier();
    lj_col(coeffs + a.off[1] + boff, sh.q + 64, v, mid);
    __builtin_amdgcn_wave_barrier();
    lj_row(mid, v, Cb);
    __builtin_amdgcn_wave_barrier();
    lj_col(coeffs + a.off[2] + boff, sh.q + 128, v, mid);
    __builtin_amdgcn_wave_barrier();
    lj_row(mid, v, Cr);
  }
  if (y > w.y1) return;
  const int nx = w.x1 + 1 - x0 < 8 ? w.x1 + 1 - x0 : 8;
  uint8_t* o = rgb + ((size_t)y * a.W + x0) * 3;
  if constexpr (SS == JDS_SS_GRAY) {
    lj_gray_store(Yv, o, nx);
  } else {
    if constexpr (C::SX == 2) {
      lj_chroma_up<SS>(sh, a, w, y, x0, 0, Cb);
      lj_chroma_up<SS>(sh, a, w, y, x0, 1, Cr);
    }
    lj_colour_store(Yv, Cb, Cr, o, nx);
  }
}

template <int SS>
LJ_KERNEL
k_jpeg_ljt(const JInvArgs a, const int16_t* __restrict__ coeffs, uint8_t* __restrict__ rgb) {
  __shared__ LjShared<SS> sh;
  lj_tile_dev<SS>(sh, a, blockIdx.x, coeffs, rgb);
}

// k_jpeg_inv_batch's contract: a workgroup finds its image in the launch's map;
// an image whose status word is set gets zeros; nothing between images is written.
template <int SS>
LJ_KERNEL
k_jpeg_ljt_batch(const JInvRec* __restrict__ recs, const JInvMap* __restrict__ map, const int nmap,
                 const uint32_t* __restrict__ status, const int16_t* __restrict__ coeffs,
                 uint8_t* __restrict__ rgb) {
  __shared__ LjShared<SS> sh;
  const int mi = jinv_find(map, nmap, (int)blockIdx.x);
  const JInvRec& r = recs[map[mi].rec];
  const int tile = (int)blockIdx.x - map[mi].tile0;
  uint8_t* o = rgb + r.rgb_off;
  if (status[r.st] != 0u) {  // (uniform)
    const JInvArgs& a = r.a;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const JWin w = lj_tile_window<SS>(a, ty, tx);
    const int rb = 3 * (w.x1 - w.X0 + 1), nb = rb * (w.y1 - w.Y0 + 1);  // inside the image: <= 3 * JI_TW * JI_TH
    for (int i = threadIdx.x; i < nb; i += JI_NT) {
      const int y = i / rb;
      o[((size_t)(w.Y0 + y) * a.W + w.X0) * 3 + (i - y * rb)] = 0;
    }
    return;
  }
  lj_tile_dev<SS>(sh, r.a, tile, coeffs + r.coef_off, o);
}

// One launch on s; nothing is uploaded or read back.
hipError_t launch_jpeg_ljt(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, hipStream_t s) {
  const dim3 grid((unsigned)(a.tiles_y * a.tiles_x)), block(JI_NT);
  if (a.ss == JDS_SS_GRAY)
    k_jpeg_ljt<JDS_SS_GRAY><<<grid, block, 0, s>>>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_420)
    k_jpeg_ljt<JDS_SS_420><<<grid, block, 0, s>>>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_422)
    k_jpeg_ljt<JDS_SS_422><<<grid, block, 0, s>>>(a, coeffs, rgb);
  else
    k_jpeg_ljt<JDS_SS_444><<<grid, block, 0, s>>>(a, coeffs, rgb);
  kmark(s, "k_jpeg_ljt<%d>", a.ss);
  return hipGetLastError();
}

// The batch: one launch per mode present (launch_jpeg_inv_batch's arguments).
hipError_t launch_jpeg_ljt_batch(const JInvRec* recs, const JInvMap* maps, const int map_off[JI_MODES],
                                 const int nmap[JI_MODES], const int tiles[JI_MODES], const uint32_t* status,
                                 const int16_t* coeffs, uint8_t* rgb, hipStream_t s) {
  const dim3 block(JI_NT);
  for (int m = 0; m < JI_MODES; ++m) {
    if (nmap[m] < 1) continue;
    const dim3 grid((unsigned)tiles[m]);
    const JInvMap* mp = maps + map_off[m];
    if (m == JDS_SS_GRAY)
      k_jpeg_ljt_batch<JDS_SS_GRAY><<<grid, block, 0, s>>>(recs, mp, nmap[m], status, coeffs, rgb);
    else if (m == JDS_SS_420)
      k_jpeg_ljt_batch<JDS_SS_420><<<grid, block, 0, s>>>(recs, mp, nmap[m], status, coeffs, rgb);
    else if (m == JDS_SS_422)
      k_jpeg_ljt_batch<JDS_SS_422><<<grid, block, 0, s>>>(recs, mp, nmap[m], status, coeffs, rgb);
    else
      k_jpeg_ljt_batch<JDS_SS_444><<<grid, block, 0, s>>>(recs, mp, nmap[m], status, coeffs, rgb);
    kmark(s, "k_jpeg_ljt_batch<%d>", m);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace jds
