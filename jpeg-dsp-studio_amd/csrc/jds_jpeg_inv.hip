// jds_jpeg_inv.hip — k_jpeg_inv: decoded coefficients of a baseline JPEG from
// elsewhere -> RGB bytes in one launch (DESIGN.md "Foreign files to pixels").
// The tile core is csrc/jds_jpeg_inv.hpp, shared with the host tile loop
// (jds_selftest_jpeg_inverse) and tools/jpeg_inv_host_san.cpp.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_internal.hpp"
#include "jds_jpeg_inv.hpp"

#pragma clang fp contract(off)

namespace jds {

// 4:2:0: 36.9 KB transpose buffer + 21.3 KB window, 4:2:2: + 35.8 KB window:
// two workgroups of 512 lanes per CU (128 VGPRs each) within the 160 KB
static_assert(sizeof(JShared<JDS_SS_422>) <= 80 * 1024 && sizeof(JShared<JDS_SS_420>) <= 80 * 1024 &&
                  sizeof(JShared<JDS_SS_444>) <= 80 * 1024,
              "two workgroups per CU");
// grayscale: the transpose buffer and one table, four workgroups per CU
static_assert(sizeof(JShared<JDS_SS_GRAY>) <= 40 * 1024, "four workgroups per CU");

// One workgroup per tile, eight lanes per block (lane v: column v, then row v).
// A block's two passes run on 8 lanes of one wave, whose LDS operations execute
// in order: wave barriers (no instruction, a scheduling fence) between them, a
// workgroup barrier only once the chroma window is complete.  a: uniform -- the
// kernel argument (k_jpeg_inv) or the image's record in global memory
// (k_jpeg_inv_batch); either way its fields arrive by scalar loads.
template <int SS>
__device__ __forceinline__ void jinv_tile_dev(JShared<SS>& sh, const JInvArgs& a, const int tile,
                                              const int16_t* __restrict__ coeffs, uint8_t* __restrict__ rgb) {
  using C = JInvCfg<SS>;
  const int tid = threadIdx.x, v = tid & 7, lb = tid >> 3;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const JWin w = jinv_tile_window<SS>(a, ty, tx);
  if (tid < 192) sh.q[tid] = a.q[tid >> 6][tid & 63];
  if (tid < JI_TW) jinv_xtap<SS>(sh, a, w, tid);
  __syncthreads();
  if constexpr (C::SX == 2) {
    const int ntask = 2 * w.ncbr * w.ncbc;
#pragma unroll 1
    for (int t = lb; t < ntask; t += JI_NB) {
      jinv_chroma_col<SS>(sh, a, w, coeffs, t, v);
      __builtin_amdgcn_wave_barrier();
      jinv_chroma_row<SS>(sh, a, w, t, v);
      __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
  }
  int by, bx;
  if (!jinv_luma_block(a, w, lb, &by, &bx)) return;  // (no barrier follows)
  double* mid = sh.mid + lb * JI_MS;
  const long long boff = ((long long)by * a.gc[0] + bx) * 64;
  const int y = by * 8 + v, x0 = bx * 8;
  double Yv[8], Cb[8], Cr[8];
  jinv_col(coeffs + a.off[0] + boff, sh.q, v, mid);
  __builtin_amdgcn_wave_barrier();
  jinv_row(mid, v, Yv);
  if constexpr (C::SX == 1) {  // 4:4:4: the co-sited chroma blocks through the same slot
    __builtin_amdgcn_wave_barrier();
    jinv_col(coeffs + a.off[1] + boff, sh.q + 64, v, mid);
    __builtin_amdgcn_wave_barrier();
    jinv_row(mid, v, Cb);
    __builtin_amdgcn_wave_barrier();
    jinv_col(coeffs + a.off[2] + boff, sh.q + 128, v, mid);
    __builtin_amdgcn_wave_barrier();
    jinv_row(mid, v, Cr);
  }
  if (y > w.y1) return;
  if constexpr (C::SX == 2) {
    jinv_chroma_up<SS>(sh, a, w, y, x0, 0, Cb);
    jinv_chroma_up<SS>(sh, a, w, y, x0, 1, Cr);
  }
  const int nx = w.x1 + 1 - x0 < 8 ? w.x1 + 1 - x0 : 8;
  jinv_colour_store(Yv, Cb, Cr, rgb + ((size_t)y * a.W + x0) * 3, nx);
}

// Grayscale: the tile's luma blocks and nothing else -- no window, no taps, no
// workgroup barrier beyond the one behind the table load.  Planes 1 and 2 do
// not exist and are never indexed (a.off[1..2], a.gr/gc[1..2] are zero and
// unread; component 0's plane starts at the coefficient base).  LDS: 37120 B
// (transpose buffer + 64 table entries), so four workgroups of 512 lanes share
// a CU's 160 KB.  The compiler reports 36 VGPRs for k_jpeg_inv<JDS_SS_GRAY> and
// 50 for k_jpeg_inv_batch<JDS_SS_GRAY> on gfx950: 8 waves per SIMD either way,
// i.e. the same four workgroups (a workgroup is 8 waves, two per SIMD).  LDS is
// the limit, not registers; no register cap is set.
template <>
__device__ __forceinline__ void jinv_tile_dev<JDS_SS_GRAY>(JShared<JDS_SS_GRAY>& sh, const JInvArgs& a, const int tile,
                                                           const int16_t* __restrict__ coeffs,
                                                           uint8_t* __restrict__ rgb) {
  const int tid = threadIdx.x, v = tid & 7, lb = tid >> 3;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  const JWin w = jinv_tile_window<JDS_SS_GRAY>(a, ty, tx);
  if (tid < 64) sh.q[tid] = a.q[0][tid];
  __syncthreads();
  int by, bx;
  if (!jinv_luma_block(a, w, lb, &by, &bx)) return;  // (no barrier follows)
  double* mid = sh.mid + lb * JI_MS;
  const long long boff = ((long long)by * a.gc[0] + bx) * 64;
  const int y = by * 8 + v, x0 = bx * 8;
  double Yv[8];
  jinv_col(coeffs + boff, sh.q, v, mid);
  __builtin_amdgcn_wave_barrier();
  jinv_row(mid, v, Yv);
  if (y > w.y1) return;
  const int nx = w.x1 + 1 - x0 < 8 ? w.x1 + 1 - x0 : 8;
  jinv_gray_store(Yv, rgb + ((size_t)y * a.W + x0) * 3, nx);
}

template <int SS>
__global__ void __launch_bounds__(JI_NT)
k_jpeg_inv(const JInvArgs a, const int16_t* __restrict__ coeffs, uint8_t* __restrict__ rgb) {
  __shared__ JShared<SS> sh;
  jinv_tile_dev<SS>(sh, a, blockIdx.x, coeffs, rgb);
}

// The tiles of a batch's images of one subsampling mode (jds_jpeg_inv.hpp
// "batches"): a workgroup finds its image in the launch's map, takes the image's
// arguments, coefficient base and pixel base from its record, and runs the tile
// core above.  An image whose status word is set (its scan data were defective:
// the word is final, every decode kernel precedes this one on the stream) gets
// zeros instead, so no host decision sits between decode and inverse.
template <int SS>
__global__ void __launch_bounds__(JI_NT)
k_jpeg_inv_batch(const JInvRec* __restrict__ recs, const JInvMap* __restrict__ map, const int nmap,
                 const uint32_t* __restrict__ status, const int16_t* __restrict__ coeffs,
                 uint8_t* __restrict__ rgb) {
  __shared__ JShared<SS> sh;
  const int mi = jinv_find(map, nmap, (int)blockIdx.x);
  const JInvRec& r = recs[map[mi].rec];
  const int tile = (int)blockIdx.x - map[mi].tile0;
  uint8_t* o = rgb + r.rgb_off;
  if (status[r.st] != 0u) {  // (uniform)
    const JInvArgs& a = r.a;
    const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
    const JWin w = jinv_tile_window<SS>(a, ty, tx);
    const int rb = 3 * (w.x1 - w.X0 + 1), nb = rb * (w.y1 - w.Y0 + 1);  // inside the image: <= 3 * JI_TW * JI_TH
    for (int i = threadIdx.x; i < nb; i += JI_NT) {
      const int y = i / rb;
      o[((size_t)(w.Y0 + y) * a.W + w.X0) * 3 + (i - y * rb)] = 0;
    }
    return;
  }
  jinv_tile_dev<SS>(sh, r.a, tile, coeffs + r.coef_off, o);
}

void jpeg_inv_constants(int* th, int* tw) {
  *th = JI_TH;
  *tw = JI_TW;
}

bool jpeg_inv_fits(const JInvArgs& a) {
  return a.ss == JDS_SS_GRAY  ? true  // (no window)
         : a.ss == JDS_SS_420 ? jinv_windows_fit<JDS_SS_420>(a)
         : a.ss == JDS_SS_422 ? jinv_windows_fit<JDS_SS_422>(a)
                              : jinv_windows_fit<JDS_SS_444>(a);
}

// One launch on s; nothing is uploaded or read back.
hipError_t launch_jpeg_inv(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, hipStream_t s) {
  const dim3 grid((unsigned)(a.tiles_y * a.tiles_x)), block(JI_NT);
  if (a.ss == JDS_SS_GRAY)
    k_jpeg_inv<JDS_SS_GRAY><<<grid, block, 0, s>>>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_420)
    k_jpeg_inv<JDS_SS_420><<<grid, block, 0, s>>>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_422)
    k_jpeg_inv<JDS_SS_422><<<grid, block, 0, s>>>(a, coeffs, rgb);
  else
    k_jpeg_inv<JDS_SS_444><<<grid, block, 0, s>>>(a, coeffs, rgb);
  kmark(s, "k_jpeg_inv<%d>", a.ss);
  return hipGetLastError();
}

// The batch: one launch per mode present.  maps: the four modes' maps one
// after another in device memory (map_off[m]: a mode's first entry; nmap[m]
// images, tiles[m] tiles).
hipError_t launch_jpeg_inv_batch(const JInvRec* recs, const JInvMap* maps, const int map_off[JI_MODES],
                                 const int nmap[JI_MODES], const int tiles[JI_MODES], const uint32_t* status,
                                 const int16_t* coeffs, uint8_t* rgb, hipStream_t s) {
  const dim3 block(JI_NT);
  for (int m = 0; m < JI_MODES; ++m) {
    if (nmap[m] < 1) continue;
    const dim3 grid((unsigned)tiles[m]);
    const JInvMap* mp = maps + map_off[m];
    if (m == JDS_SS_GRAY)
      k_jpeg_inv_batch<JDS_SS_GRAY><<<grid, block, 0, s>>>(recs, mp, nmap[m], status, coeffs, rgb);
    else if (m == JDS_SS_420)
      k_jpeg_inv_batch<JDS_SS_420><<<grid, block, 0, s>>>(recs, mp, nmap[m], status, coeffs, rgb);
    else if (m == JDS_SS_422)
      k_jpeg_inv_batch<JDS_SS_422><<<grid, block, 0, s>>>(recs, mp, nmap[m], status, coeffs, rgb);
    else
      k_jpeg_inv_batch<JDS_SS_444><<<grid, block, 0, s>>>(recs, mp, nmap[m], status, coeffs, rgb);
    kmark(s, "k_jpeg_inv_batch<%d>", m);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

void jpeg_inv_host(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb) {
  if (a.ss == JDS_SS_GRAY)
    jinv_host_image<JDS_SS_GRAY>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_420)
    jinv_host_image<JDS_SS_420>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_422)
    jinv_host_image<JDS_SS_422>(a, coeffs, rgb);
  else
    jinv_host_image<JDS_SS_444>(a, coeffs, rgb);
}

}  // namespace jds
