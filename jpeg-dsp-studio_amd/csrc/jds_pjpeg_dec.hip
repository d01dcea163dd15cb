// jds_pjpeg_dec.hip — the entropy decode of progressive files (DESIGN.md
// "Progressive files"): k_pjpeg_chains walks the chains of a batch, one chain
// per workgroup of one wave.  Lane 0 runs the sequential Annex-G walk of
// csrc/jds_pjpeg_dec.hpp (shared with the host model); the wave's other lanes
// only stage: before every scan they copy the scan's decode tables (and once
// the file's MCU record) into LDS, where the walk's table lookups are a
// dependent load per symbol.  A batch has 4 chains per colour file, far fewer
// than the device has wave slots, so a wave per chain costs nothing and keeps
// the walking lane free of divergence with other chains.
//
// The scan bytes are read through 8-byte aligned words of the batch's upload
// (one global load per eight bytes); coefficients are plain 16-bit loads and
// stores of the chain's own entries.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_internal.hpp"
#include "jds_pjpeg_dec.hpp"

namespace jds {

// The batch's upload as a byte source: base is 8-byte aligned and the upload is
// a multiple of 8 bytes long, so the word that holds an in-range byte is the
// upload's own.
struct PjWordSrc {
  const unsigned long long* w;
  int64_t n;
  mutable int64_t at = -1;
  mutable unsigned long long cur = 0;
  __device__ __forceinline__ uint32_t byte(int64_t i) const {
    const int64_t k = i >> 3;
    if (k != at) {
      cur = w[k];
      at = k;
    }
    return (uint32_t)(cur >> (8 * (int)(i & 7))) & 0xFFu;
  }
};

constexpr int PJ_WAVE = 64;

__global__ __launch_bounds__(PJ_WAVE) void k_pjpeg_chains(const unsigned long long* files, long long files_bytes,
                                                         const PjChain* chains, const PjScan* scans,
                                                         const HuffDecTab* tabs, const HdMcu* mcus, int16_t* coeffs,
                                                         uint32_t* status, unsigned long long* ticks) {
  __shared__ HuffDecTab s_tab[3];
  __shared__ HdMcu s_m;
  __shared__ uint32_t s_st;
  const int tid = threadIdx.x;
  const PjChain ch = chains[blockIdx.x];
  {
    const uint32_t* src = (const uint32_t*)(mcus + ch.file);
    uint32_t* dst = (uint32_t*)&s_m;
    for (int i = tid; i < (int)(sizeof(HdMcu) / 4); i += PJ_WAVE) dst[i] = src[i];
  }
  if (tid == 0) s_st = 0;
  for (int i = 0; i < ch.nscans; ++i) {
    const PjScan sc = scans[ch.scan0 + i];
    __syncthreads();  // (the previous scan's walk is over: its tables may go)
    for (int j = 0; j < 3; ++j)
      if (sc.tab[j] >= 0) {
        const uint32_t* src = (const uint32_t*)(tabs + sc.tab[j]);
        uint32_t* dst = (uint32_t*)&s_tab[j];
        for (int k = tid; k < (int)(sizeof(HuffDecTab) / 4); k += PJ_WAVE) dst[k] = src[k];
      }
    __syncthreads();
    if (tid == 0) {
      uint32_t st = HD_BAD_HEADER;
      const unsigned long long t0 = ticks ? wall_clock64() : 0ull;
      // (the host builds every range inside the upload; a descriptor outside it decodes nothing)
      if (sc.data_off >= 0 && sc.nbytes >= 0 && sc.data_off + sc.nbytes <= files_bytes) {
        const HuffDecTab* t[3] = {sc.tab[0] >= 0 ? &s_tab[0] : nullptr, sc.tab[1] >= 0 ? &s_tab[1] : nullptr,
                                  sc.tab[2] >= 0 ? &s_tab[2] : nullptr};
        const PjWordSrc src{files, (int64_t)files_bytes};
        st = hd_pjpeg_scan(src, t, sc, s_m, PjCoefSink{coeffs});
      }
      s_st = st;
      if (ticks) ticks[ch.scan0 + i] = wall_clock64() - t0;  // (a profiled context: the scan's walk time)
    }
    __syncthreads();
    if (s_st) break;  // (uniform: the defect ends the chain)
  }
  if (tid == 0 && s_st) atomicOr(&status[ch.file], s_st);
}

hipError_t launch_pjpeg_chains(const uint8_t* files, long long files_bytes, const PjChain* chains, int nchains,
                               const PjScan* scans, const HuffDecTab* tabs, const HdMcu* mcus, int16_t* coeffs,
                               uint32_t* status, unsigned long long* ticks, hipStream_t s) {
  if (nchains <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_pjpeg_chains, dim3((unsigned)nchains), dim3(PJ_WAVE), 0, s, (const unsigned long long*)files,
                     files_bytes, chains, scans, tabs, mcus, coeffs, status, ticks);
  kmark(s, "k_pjpeg_chains");
  return hipGetLastError();
}

}  // namespace jds
