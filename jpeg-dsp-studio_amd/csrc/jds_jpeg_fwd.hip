// jds_jpeg_fwd.hip — k_jpeg_fwd: RGB (or gray) bytes -> the quantised
// coefficients libjpeg's default compressor gives, in jds_decode_jpeg's planar
// layout, in one launch (DESIGN.md "libjpeg encoding").  The tile core is
// csrc/jds_jpeg_fwd.hpp, shared with the host tile loop
// (jds_selftest_jpeg_forward) and tools/jpeg_fwd_san.cpp; arguments, tile,
// records and maps are k_jpeg_inv's (csrc/jds_jpeg_inv.hpp).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_internal.hpp"
#include "jds_jpeg_fwd.hpp"

namespace jds {

// The sample planes are int16 and the passes run in place, so a workgroup keeps
// 9 KB of luma, 5 KB (4:2:0), 10 KB (4:2:2) or 18 KB (4:4:4) of chroma and
// 1.5 KB of tables: four workgroups of 512 lanes (all 32 wave slots of a CU) take
// at most 114 KB of the 160 KB.  Registers: four workgroups are 8 waves per SIMD,
// i.e. at most 64 VGPRs; the instantiations take 20 to 45 and no scratch, so
// what JF_KERNEL asks for costs nothing.
static_assert(sizeof(JfShared<JDS_SS_422>) <= 40 * 1024 && sizeof(JfShared<JDS_SS_420>) <= 40 * 1024 &&
                  sizeof(JfShared<JDS_SS_444>) <= 40 * 1024 && sizeof(JfShared<JDS_SS_GRAY>) <= 40 * 1024,
              "the LDS of four workgroups per CU");
#define JF_KERNEL __global__ void __launch_bounds__(JI_NT) __attribute__((amdgpu_waves_per_eu(8, 8)))

// One workgroup per tile.  Staging: lane l converts patch l (and l + JI_NT where
// a patch is one pixel row).  Then eight lanes per block (lane v: row v, then
// column v, then row v out): the block's passes run on 8 lanes of one wave,
// whose LDS operations execute in order, so wave barriers separate them; the
// workgroup barrier stands between the staging and the blocks.
// a: uniform (the kernel argument or the image's record).
template <int SS>
__device__ __forceinline__ void jf_tile_dev(JfShared<SS>& sh, const JInvArgs& a, const int tile,
                                            const uint8_t* __restrict__ img, int16_t* __restrict__ coeffs) {
  using C = JfCfg<SS>;
  const int tid = threadIdx.x, v = tid & 7, lb = tid >> 3;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const JWin w = jf_tile_window(a, ty, tx);
  if (tid < 64 * C::NPLANES) {
    const int q = a.q[tid >> 6][tid & 63];
    sh.q[tid] = q;
    sh.r[tid] = jf_recip(q);
  }
#pragma unroll 1
  for (int p = tid; p < C::NPATCH; p += JI_NT) jf_stage<SS>(sh, a, w, img, p);
  __syncthreads();
#pragma unroll 1
  for (int t = lb; t < C::NTASK; t += JI_NB) {
    const JfTask k = jf_task<SS>(sh, a, w, t);
    if (k.ok) jf_rows(k, v);
    __builtin_amdgcn_wave_barrier();
    if (k.ok) jf_cols(k, sh.q, sh.r, v);
    __builtin_amdgcn_wave_barrier();
    if (k.ok) jf_out(k, coeffs, v);
  }
}

template <int SS>
JF_KERNEL
k_jpeg_fwd(const JInvArgs a, const uint8_t* __restrict__ img, int16_t* __restrict__ coeffs) {
  __shared__ JfShared<SS> sh;
  jf_tile_dev<SS>(sh, a, blockIdx.x, img, coeffs);
}

// k_jpeg_inv_batch's map walk: a workgroup finds its image in the launch's map.
// r.rgb_off: the image's first byte from img (any offset); r.st is not used.
template <int SS>
JF_KERNEL
k_jpeg_fwd_batch(const JInvRec* __restrict__ recs, const JInvMap* __restrict__ map, const int nmap,
                 const uint8_t* __restrict__ img, int16_t* __restrict__ coeffs) {
  __shared__ JfShared<SS> sh;
  const int mi = jinv_find(map, nmap, (int)blockIdx.x);
  const JInvRec& r = recs[map[mi].rec];
  jf_tile_dev<SS>(sh, r.a, (int)blockIdx.x - map[mi].tile0, img + r.rgb_off, coeffs + r.coef_off);
}

// One launch on s; nothing is uploaded or read back.
hipError_t launch_jpeg_fwd(const JInvArgs& a, const uint8_t* img, int16_t* coeffs, hipStream_t s) {
  const dim3 grid((unsigned)(a.tiles_y * a.tiles_x)), block(JI_NT);
  if (a.ss == JDS_SS_GRAY)
    k_jpeg_fwd<JDS_SS_GRAY><<<grid, block, 0, s>>>(a, img, coeffs);
  else if (a.ss == JDS_SS_420)
    k_jpeg_fwd<JDS_SS_420><<<grid, block, 0, s>>>(a, img, coeffs);
  else if (a.ss == JDS_SS_422)
    k_jpeg_fwd<JDS_SS_422><<<grid, block, 0, s>>>(a, img, coeffs);
  else
    k_jpeg_fwd<JDS_SS_444><<<grid, block, 0, s>>>(a, img, coeffs);
  kmark(s, "k_jpeg_fwd<%d>", a.ss);
  return hipGetLastError();
}

// The batch: one launch per mode present (launch_jpeg_inv_batch's arguments).
hipError_t launch_jpeg_fwd_batch(const JInvRec* recs, const JInvMap* maps, const int map_off[JI_MODES],
                                 const int nmap[JI_MODES], const int tiles[JI_MODES], const uint8_t* img,
                                 int16_t* coeffs, hipStream_t s) {
  const dim3 block(JI_NT);
  for (int m = 0; m < JI_MODES; ++m) {
    if (nmap[m] < 1) continue;
    const dim3 grid((unsigned)tiles[m]);
    const JInvMap* mp = maps + map_off[m];
    if (m == JDS_SS_GRAY)
      k_jpeg_fwd_batch<JDS_SS_GRAY><<<grid, block, 0, s>>>(recs, mp, nmap[m], img, coeffs);
    else if (m == JDS_SS_420)
      k_jpeg_fwd_batch<JDS_SS_420><<<grid, block, 0, s>>>(recs, mp, nmap[m], img, coeffs);
    else if (m == JDS_SS_422)
      k_jpeg_fwd_batch<JDS_SS_422><<<grid, block, 0, s>>>(recs, mp, nmap[m], img, coeffs);
    else
      k_jpeg_fwd_batch<JDS_SS_444><<<grid, block, 0, s>>>(recs, mp, nmap[m], img, coeffs);
    kmark(s, "k_jpeg_fwd_batch<%d>", m);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace jds
