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

// One workgroup per tile, eight lanes per block (lane v: column v, then row v).
// A block's two passes run on 8 lanes of one wave, whose LDS operations execute
// in order: wave barriers (no instruction, a scheduling fence) between them, a
// workgroup barrier only once the chroma window is complete.
template <int SS>
__global__ void __launch_bounds__(JI_NT)
k_jpeg_inv(const JInvArgs a, const int16_t* __restrict__ coeffs, uint8_t* __restrict__ rgb) {
  using C = JInvCfg<SS>;
  __shared__ JShared<SS> sh;
  const int tid = threadIdx.x, v = tid & 7, lb = tid >> 3;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
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

void jpeg_inv_constants(int* th, int* tw) {
  *th = JI_TH;
  *tw = JI_TW;
}

bool jpeg_inv_fits(const JInvArgs& a) {
  return a.ss == JDS_SS_420 ? jinv_windows_fit<JDS_SS_420>(a)
         : a.ss == JDS_SS_422 ? jinv_windows_fit<JDS_SS_422>(a)
                              : jinv_windows_fit<JDS_SS_444>(a);
}

// One launch on s; nothing is uploaded or read back.
hipError_t launch_jpeg_inv(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, hipStream_t s) {
  const dim3 grid((unsigned)(a.tiles_y * a.tiles_x)), block(JI_NT);
  if (a.ss == JDS_SS_420)
    k_jpeg_inv<JDS_SS_420><<<grid, block, 0, s>>>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_422)
    k_jpeg_inv<JDS_SS_422><<<grid, block, 0, s>>>(a, coeffs, rgb);
  else
    k_jpeg_inv<JDS_SS_444><<<grid, block, 0, s>>>(a, coeffs, rgb);
  kmark(s, "k_jpeg_inv<%d>", a.ss);
  return hipGetLastError();
}

void jpeg_inv_host(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb) {
  if (a.ss == JDS_SS_420)
    jinv_host_image<JDS_SS_420>(a, coeffs, rgb);
  else if (a.ss == JDS_SS_422)
    jinv_host_image<JDS_SS_422>(a, coeffs, rgb);
  else
    jinv_host_image<JDS_SS_444>(a, coeffs, rgb);
}

}  // namespace jds
