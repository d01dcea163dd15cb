// jds_entropy_dec.hip — baseline JPEG entropy DECODING: the scans of the JFIF
// files jds_entropy.hip writes (or any baseline file of that profile) back to
// all_quantized_coeffs.  A Huffman stream without restart markers has no known
// codeword boundaries, so the decode is self-synchronising (Weissenberger &
// Schmidt, "Massively Parallel Huffman Decoding on GPUs", and its JPEG
// follow-up): every scan is cut into subsequences of DEC_S bits, one lane
// decodes each from the guess (first bit, DC expected), exit states are handed
// to the next subsequence, and lanes whose entry changed decode again until
// none changes.  The per-subsequence routine is csrc/jds_huffdec.hpp, shared
// with the host model.
//
//   k_dec_find   plan path: marker search over every frame's file.
//   k_dec_hdr    plan path, one workgroup per frame: header == the plan's own
//                header template; the marker list -> the three scans' byte ranges.
//   k_dec_sync   one workgroup per DEC_G subsequences of one scan, their bytes
//                staged in LDS: decode, then propagate inside the workgroup
//                through LDS until its entries settle.  Across workgroups the hand-off happens
//                BETWEEN launches: a workgroup's last exit state goes to a
//                double-buffered array the next launch reads; no kernel waits
//                on another workgroup.  The host reads a "changed" counter
//                after each launch and stops at zero (at most one launch per
//                workgroup of the longest scan).
//   k_dec_prefix per scan: exclusive prefix of the subsequences' block counts.
//   k_dec_write  every lane decodes again from its settled entry and stores the
//                coefficients de-zigzagged (per coefficient: a block that spans
//                subsequences is written by several lanes); judges the scan.
//   k_dec_dc     per scan: the DC differences -> values (inclusive sum, judged
//                against int16).
// Scans with restart intervals need none of this: k_rst_scan / k_dec_rst at
// the end of the file.
//
// Interleaved scans (jds_decode_jpeg; DESIGN.md "Interleaved scans"): k_dec_sync,
// k_dec_write and k_dec_rst have a second instantiation, <true>, whose decoder
// state carries the block's slot in the MCU and whose tables are chosen per slot
// from the MCU descriptor (HdMcu, in LDS beside all four decode tables).  Its
// write pass places blocks through hd_il_place, drops the ones that pad the
// image to whole MCUs, and sends every DC difference to a scan-order staging
// array; k_dec_dc_mcu sums a component's differences there and places the
// values.  The <false> instantiations are the code described above.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "jds_huffdec.hpp"
#include "jds_internal.hpp"

namespace jds {

#ifndef JDS_DEC_S
#define JDS_DEC_S 1024  // A/B builds: tools/build_variant.py
#endif
#ifndef JDS_DEC_G
#define JDS_DEC_G 256
#endif
constexpr int DEC_S = JDS_DEC_S;  // bits per subsequence
constexpr int DEC_G = JDS_DEC_G;  // subsequences (lanes) per workgroup
static_assert(DEC_S % 8 == 0 && DEC_S >= 64, "a symbol (<= 27 bits + 4 stuffed bytes) ends inside the next subsequence");

void dec_constants(int* s, int* g) {
  *s = DEC_S;
  *g = DEC_G;
}

// Fills nsub / grp0 / ngrp; returns the number of workgroups, *max_ngrp the
// longest scan's.  nblocks == 0 marks a skipped scan (no workgroups).
long long dec_layout(DecScan* sc, int nscans, int* max_ngrp) {
  long long g = 0;
  int mx = 0;
  for (int i = 0; i < nscans; ++i) {
    const long long nbits = sc[i].nbytes * 8;
    long long nsub = sc[i].nblocks ? (nbits + DEC_S - 1) / DEC_S : 0;
    if (sc[i].nblocks && nsub == 0) nsub = 1;  // an empty scan still gets judged
    if (nsub > 0x7fffffffll || g > 0x7fffffffll) return -1;
    sc[i].nsub = (int)nsub;
    sc[i].grp0 = (int)g;
    sc[i].ngrp = (int)((nsub + DEC_G - 1) / DEC_G);
    g += sc[i].ngrp;
    mx = sc[i].ngrp > mx ? sc[i].ngrp : mx;
  }
  *max_ngrp = mx;
  return g;
}

// scratch layout (bytes, 8-aligned parts): entry, exit (u64 per slot), the two
// hand-off buffers (u64 per workgroup), blocks / first block (u32 per slot),
// scans, workgroup -> scan, counters
struct DecScratch {
  unsigned long long *entry, *exitv, *gx[2];
  unsigned *nblk, *blk0;
  DecScan* scans;
  int* grp_scan;
  unsigned* changed;
  size_t bytes;
};

static size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

DecScratch dec_scratch(void* base, long long ngroups, int nscans) {
  DecScratch s{};
  const size_t slots = (size_t)ngroups * DEC_G;
  char* p = (char*)base;
  size_t o = 0;
  s.entry = (unsigned long long*)(p + o); o += 8 * slots;
  s.exitv = (unsigned long long*)(p + o); o += 8 * slots;
  s.gx[0] = (unsigned long long*)(p + o); o += 8 * (size_t)(ngroups + 1);
  s.gx[1] = (unsigned long long*)(p + o); o += 8 * (size_t)(ngroups + 1);
  s.nblk = (unsigned*)(p + o); o += up8(4 * slots);
  s.blk0 = (unsigned*)(p + o); o += up8(4 * slots);
  s.scans = (DecScan*)(p + o); o += up8(sizeof(DecScan) * (size_t)nscans);
  s.grp_scan = (int*)(p + o); o += up8(4 * (size_t)(ngroups + 1));
  s.changed = (unsigned*)(p + o); o += 16;
  s.bytes = o;
  return s;
}

size_t dec_scratch_bytes(long long ngroups, int nscans) { return dec_scratch(nullptr, ngroups, nscans).bytes; }

// ------------------------------------------------------------ kernels --

constexpr int DEC_SOS = 10;

// Marker search of the plan path: 0xFF followed by anything but the stuffed
// 0x00, from the header's end on (scan data hold no other 0xFF pairs, so a
// well-formed file has exactly four: three SOS and EOI).  Grid (pieces, frames):
// a thread scans DEC_FIND_B bytes in 16-byte pieces aligned in memory (whole
// pieces inside [hl, len) as one load, ragged ends by bytes, nothing outside the
// file) and appends what it finds to the frame's list (cnt[f], pos[8 f ..]).
constexpr int DEC_FIND_B = 64;

__global__ void __launch_bounds__(256) k_dec_find(const uint8_t* __restrict__ files, long long stride,
                                                  const unsigned long long* __restrict__ lengths, int hl,
                                                  int* __restrict__ cnt, long long* __restrict__ pos) {
  const int f = blockIdx.y;
  const unsigned long long len64 = lengths[f];
  if (len64 < (unsigned long long)(hl + 3 * DEC_SOS + 2) || len64 > (unsigned long long)stride) return;
  const long long len = (long long)len64;
  const uint8_t* d = files + (long long)f * stride;
  const long long a0 = hl - (long long)((uintptr_t)(d + hl) & 15u);  // frame-relative start of the piece holding byte hl
  const long long base = a0 + ((long long)blockIdx.x * 256 + threadIdx.x) * DEC_FIND_B;
  for (int c = 0; c < DEC_FIND_B / 16; ++c) {
    const long long g = base + 16 * c;
    if (g + 1 >= len) return;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    if (g >= hl && g + 16 <= len) {
      const uint4 v = *reinterpret_cast<const uint4*>(d + g);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 16; ++j)
        if (g + j >= hl && g + j < len) w[j >> 2] |= (uint32_t)d[g + j] << (8 * (j & 3));
    }
    bool ff = false;  // some byte is 0xFF: a zero byte of ~w
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t x = ~w[k];
      ff = ff || (((x - 0x01010101u) & ~x & 0x80808080u) != 0u);
    }
    if (!ff) continue;
    const uint32_t nx = g + 16 < len ? (uint32_t)d[g + 16] : 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const uint32_t bj = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
      const uint32_t bn = j < 15 ? (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu : nx;
      if (bj == 0xFFu && bn != 0u && g + j >= hl && g + j + 1 < len) {
        const int k = atomicAdd(&cnt[f], 1);
        if (k < 8) pos[8 * (long long)f + k] = g + j;
      }
    }
  }
}

// Header check of one frame (plan path) and its scans' byte ranges from the
// marker list.  scaninfo[6 f ..]: (offset, length) of the Y, Cb, Cr scans
// within the frame's file.
__global__ void __launch_bounds__(256) k_dec_hdr(const uint8_t* __restrict__ files, long long stride,
                                                 const unsigned long long* __restrict__ lengths,
                                                 const uint8_t* __restrict__ hdr, int hl,
                                                 const int* __restrict__ cnt, const long long* __restrict__ mpos,
                                                 long long* __restrict__ scaninfo, uint32_t* __restrict__ status) {
  const int f = blockIdx.x, t = threadIdx.x;
  const unsigned long long len64 = lengths[f];
  const uint8_t* d = files + (long long)f * stride;
  if (len64 < (unsigned long long)(hl + 3 * DEC_SOS + 2) || len64 > (unsigned long long)stride) {  // (uniform)
    if (t == 0) status[f] = HD_BAD_HEADER;
    return;
  }
  const long long len = (long long)len64;
  int bad = 0;
  for (int i = t; i < hl; i += 256) bad |= d[i] != hdr[(long long)f * hl + i];
  bad = __syncthreads_or(bad);
  if (t != 0) return;
  long long pos[4] = {0, 0, 0, 0};
  if (cnt[f] != 4) {
    bad = 1;
  } else {
    for (int i = 0; i < 4; ++i) pos[i] = mpos[8 * (long long)f + i];
    for (int i = 0; i < 4; ++i)  // (four entries)
      for (int j = i + 1; j < 4; ++j)
        if (pos[j] < pos[i]) {
          const long long x = pos[i];
          pos[i] = pos[j];
          pos[j] = x;
        }
    bad |= pos[0] != hl || pos[3] != len - 2 || d[len - 1] != 0xD9;
    for (int s2 = 0; s2 < 3 && !bad; ++s2) {
      const uint8_t sos[DEC_SOS] = {0xFF, 0xDA, 0x00, 0x08, 0x01, (uint8_t)(s2 + 1), (uint8_t)(s2 == 0 ? 0x00 : 0x11),
                                    0x00, 0x3F, 0x00};
      if (pos[s2] + DEC_SOS > pos[s2 + 1]) {
        bad = 1;
        break;
      }
      for (int i = 0; i < DEC_SOS; ++i) bad |= d[pos[s2] + i] != sos[i];
    }
  }
  for (int s2 = 0; s2 < 3; ++s2) {
    scaninfo[6 * f + 2 * s2] = bad ? 0 : pos[s2] + DEC_SOS;
    scaninfo[6 * f + 2 * s2 + 1] = bad ? 0 : pos[s2 + 1] - (pos[s2] + DEC_SOS);
  }
  status[f] = bad ? HD_BAD_HEADER : 0u;
}

// A workgroup's part of its scan in LDS: the bytes of its DEC_G subsequences
// and DEC_TAIL more (a symbol that starts in the last subsequence reads up to
// ten bytes from its first one).  Staged with coalesced dword loads -- whole
// dwords inside the scan, single bytes at its ragged ends, nothing outside it
// -- from the dword-aligned address at or below the first byte, so LDS dword t
// is global dword t.  Each lane's 128-byte row is padded by one dword: rows
// start 33 dwords apart and the lanes of a wave, all reading at about the same
// offset into their own rows, fall on distinct banks (unpadded, every lane of
// a wave hits the same bank).
constexpr int DEC_TAIL = 16;
constexpr int DEC_ROW = DEC_S / 32;                              // dwords per subsequence
constexpr int DEC_WIN = DEC_G * DEC_ROW + DEC_TAIL / 4 + 1;      // dwords staged (+1: the alignment shift)
constexpr int DEC_LDS = DEC_WIN + DEC_WIN / DEC_ROW + 1;         // with the row padding
static_assert(DEC_S % 32 == 0, "rows of whole dwords");

__device__ __forceinline__ int dec_lds_idx(int q) { return q + q / DEC_ROW; }

struct DecLdsSrc {
  const uint32_t* lds;
  const uint8_t* d;  // the scan's bytes (global)
  int64_t n;
  int64_t o0;        // scan-relative byte of LDS dword 0 (may be negative: the alignment shift)
  __device__ __forceinline__ uint32_t byte(int64_t i) const { return d[i]; }
  __device__ __forceinline__ void bytes10(int64_t b, uint64_t& lo, uint64_t& hi) const {
    const int64_t o = b - o0;
    if (o >= 0 && o + 16 <= 4 * (int64_t)DEC_WIN) {
      const int q = (int)(o >> 2), sh = 8 * (int)(o & 3);
      const uint64_t w0 = lds[dec_lds_idx(q)], w1 = lds[dec_lds_idx(q + 1)], w2 = lds[dec_lds_idx(q + 2)],
                     w3 = lds[dec_lds_idx(q + 3)];
      const uint64_t a = w0 | (w1 << 32), c = w2 | (w3 << 32);
      lo = sh ? (a >> sh) | (c << (64 - sh)) : a;
      hi = c >> sh;
    } else {  // outside the staged window (a hand-off far past this workgroup's bytes): global bytes
      lo = 0;
      hi = 0;
      for (int j = 0; j < 8; ++j)
        if (b + j < n) lo |= (uint64_t)d[b + j] << (8 * j);
      for (int j = 0; j < 2; ++j)
        if (b + 8 + j < n) hi |= (uint64_t)d[b + 8 + j] << (8 * j);
    }
  }
};

// Stage the workgroup's window (every thread of the workgroup; barrier after).
__device__ __forceinline__ DecLdsSrc dec_stage(uint32_t* s_win, const uint8_t* d, int64_t n, int64_t first_byte) {
  const int mis = (int)((uintptr_t)(d + first_byte) & 3u);
  const int64_t o0 = first_byte - mis;
  for (int t = threadIdx.x; t < DEC_WIN; t += DEC_G) {
    const int64_t g = o0 + 4 * (int64_t)t;
    uint32_t v = 0;
    if (g >= 0 && g + 4 <= n) {
      v = *reinterpret_cast<const uint32_t*>(d + g);
    } else {
      for (int j = 0; j < 4; ++j)
        if (g + j >= 0 && g + j < n) v |= (uint32_t)d[g + j] << (8 * j);
    }
    s_win[dec_lds_idx(t)] = v;
  }
  return DecLdsSrc{s_win, d, n, o0};
}

// the scan's two decode tables -> LDS (words; every thread of the workgroup)
__device__ __forceinline__ void load_tabs(HuffDecTab* s_tab, const HuffDecTab* __restrict__ tabs, int dc, int ac) {
  static_assert(sizeof(HuffDecTab) % 4 == 0, "word copy");
  constexpr int NW = (int)(sizeof(HuffDecTab) / 4);
  const uint32_t* a = reinterpret_cast<const uint32_t*>(tabs + dc);
  const uint32_t* b = reinterpret_cast<const uint32_t*>(tabs + ac);
  uint32_t* o = reinterpret_cast<uint32_t*>(s_tab);
  for (int i = threadIdx.x; i < NW; i += DEC_G) {
    o[i] = a[i];
    o[NW + i] = b[i];
  }
}

// all four decode tables and the MCU descriptor of an interleaved scan -> LDS
__device__ __forceinline__ void load_il(HuffDecTab* s_tab, uint32_t* s_mcu, const HuffDecTab* __restrict__ tabs,
                                        const HdMcu* __restrict__ mcu, int nthr) {
  static_assert(sizeof(HdMcu) % 4 == 0, "word copy");
  constexpr int NW = (int)(4 * sizeof(HuffDecTab) / 4), NM = (int)(sizeof(HdMcu) / 4);
  const uint32_t* a = reinterpret_cast<const uint32_t*>(tabs);
  const uint32_t* b = reinterpret_cast<const uint32_t*>(mcu);
  uint32_t* o = reinterpret_cast<uint32_t*>(s_tab);
  for (int i = threadIdx.x; i < NW; i += nthr) o[i] = a[i];
  for (int i = threadIdx.x; i < NM; i += nthr) s_mcu[i] = b[i];
}

constexpr int MCU_W = (int)(sizeof(HdMcu) / 4);

// IL: the scan is interleaved (state with slot, tables per slot from the MCU
// descriptor `mcu`); the non-interleaved instantiation ignores `mcu`.
template <bool IL>
__global__ void __launch_bounds__(DEC_G) k_dec_sync(const uint8_t* __restrict__ files,
                                                    const DecScan* __restrict__ scans,
                                                    const int* __restrict__ grp_scan,
                                                    const HuffDecTab* __restrict__ tabs,
                                                    unsigned long long* __restrict__ entry,
                                                    unsigned long long* __restrict__ exitv,
                                                    unsigned* __restrict__ nblk,
                                                    const unsigned long long* __restrict__ gx_in,
                                                    unsigned long long* __restrict__ gx_out,
                                                    unsigned* __restrict__ changed, const int round,
                                                    const HdMcu* __restrict__ mcu) {
  __shared__ HuffDecTab s_tab[IL ? 4 : 2];
  __shared__ __attribute__((aligned(8))) uint32_t s_mcu[IL ? MCU_W : 2];
  __shared__ uint32_t s_win[DEC_LDS];
  __shared__ unsigned long long s_exit[DEC_G];
  __shared__ int s_go;
  const int g = blockIdx.x, t = threadIdx.x;
  const DecScan sc = scans[grp_scan[g]];
  const int gl = g - sc.grp0;
  const long long i = (long long)gl * DEC_G + t;  // subsequence within the scan
  const size_t slot = (size_t)g * DEC_G + t;
  const bool live = i < sc.nsub;
  const uint8_t* d = files + sc.data_off;
  const long long n = sc.nbytes;
  unsigned long long ent, ex = HD_NONE;
  unsigned nb = 0;
  bool need;
  if (round == 0) {
    ent = live ? (i == 0 ? 0ull : hd_guess(HdMemSrc{d, n}, i * DEC_S)) : HD_NONE;
    need = live;
  } else {
    // only a changed hand-off from the previous workgroup of the scan restarts this one
    ent = entry[slot];
    ex = exitv[slot];
    nb = nblk[slot];
    need = false;
    if (t == 0) {
      if (gl > 0) {
        const unsigned long long c = gx_in[g - 1];
        if (c != HD_NONE && c != ent) {
          ent = c;
          need = true;
        }
      }
      s_go = need;
    }
    __syncthreads();
    if (!s_go) {  // (uniform)
      if (t == 0) gx_out[g] = gx_in[g];
      return;
    }
  }
  if constexpr (IL)
    load_il(s_tab, s_mcu, tabs + 4 * sc.file, mcu + sc.file, DEC_G);
  else
    load_tabs(s_tab, tabs, sc.dc_tab, sc.ac_tab);
  const DecLdsSrc src = dec_stage(s_win, d, n, (long long)gl * DEC_G * (DEC_S / 8));
  __syncthreads();
  // entries 0..r of the workgroup are settled after iteration r: at most DEC_G iterations
  for (int it = 0; it <= DEC_G; ++it) {
    if (need) {
      if constexpr (IL)
        ex = hd_sync_lane(src, HdIl{s_tab, reinterpret_cast<const HdMcu*>(s_mcu)}, ent,
                          (unsigned long long)(i + 1) * DEC_S, nb);
      else
        ex = hd_sync_lane(src, HdPlain{&s_tab[0], &s_tab[1]}, ent, (unsigned long long)(i + 1) * DEC_S, nb);
    }
    s_exit[t] = ex;
    __syncthreads();
    need = false;
    if (live && t > 0) {
      const unsigned long long c = s_exit[t - 1];
      if (c != HD_NONE && c != ent) {
        ent = c;
        need = true;
      }
    }
    if (!__syncthreads_or(need)) break;
  }
  entry[slot] = ent;
  exitv[slot] = ex;
  nblk[slot] = live ? nb : 0u;
  if (t == DEC_G - 1) {
    if (gl < sc.ngrp - 1 && (round == 0 || ex != gx_in[g])) atomicAdd(changed, 1u);
    gx_out[g] = ex;
  }
}

// Exclusive prefix of a scan's per-subsequence block counts (one 1024-thread
// workgroup per scan).
__global__ void __launch_bounds__(1024) k_dec_prefix(const DecScan* __restrict__ scans,
                                                     const unsigned* __restrict__ nblk,
                                                     unsigned* __restrict__ blk0) {
  __shared__ unsigned long long s_w[16];
  const DecScan sc = scans[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long long n = (long long)sc.ngrp * DEC_G, g0 = (long long)sc.grp0 * DEC_G;
  const long long C = (n + 1023) / 1024, i0 = t * C, i1 = min(n, i0 + C);
  unsigned long long loc = 0ull;
  for (long long i = i0; i < i1; ++i) loc += nblk[g0 + i];
  unsigned long long inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  unsigned long long run = inc - loc;
  for (int w = 0; w < wv; ++w) run += s_w[w];
  for (long long i = i0; i < i1; ++i) {
    const unsigned v = nblk[g0 + i];
    blk0[g0 + i] = (unsigned)(run < 0xffffffffull ? run : 0xffffffffull);  // beyond any scan's block count
    run += v;
  }
}

struct DecSink {
  int16_t* out;
  const uint8_t* zz;
  __device__ __forceinline__ void operator()(int64_t blk, int k, int v) const { out[blk * 64 + zz[k]] = (int16_t)v; }
};

__constant__ uint8_t c_dec_zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                     12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                     58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// IL: blocks go through HdIlSink (planar placement, padding dropped, DC
// differences to the staging array dcs); the other instantiation ignores mcu / dcs.
template <bool IL>
__global__ void __launch_bounds__(DEC_G) k_dec_write(const uint8_t* __restrict__ files,
                                                     const DecScan* __restrict__ scans,
                                                     const int* __restrict__ grp_scan,
                                                     const HuffDecTab* __restrict__ tabs,
                                                     const unsigned long long* __restrict__ entry,
                                                     const unsigned* __restrict__ blk0, int16_t* __restrict__ coeffs,
                                                     uint32_t* __restrict__ status, const HdMcu* __restrict__ mcu,
                                                     int16_t* __restrict__ dcs) {
  __shared__ HuffDecTab s_tab[IL ? 4 : 2];
  __shared__ __attribute__((aligned(8))) uint32_t s_mcu[IL ? MCU_W : 2];
  __shared__ uint32_t s_win[DEC_LDS];
  __shared__ uint8_t s_zz[64];
  const int g = blockIdx.x, t = threadIdx.x;
  const DecScan sc = scans[grp_scan[g]];
  const long long i = (long long)(g - sc.grp0) * DEC_G + t;
  const size_t slot = (size_t)g * DEC_G + t;
  if constexpr (IL)
    load_il(s_tab, s_mcu, tabs + 4 * sc.file, mcu + sc.file, DEC_G);
  else
    load_tabs(s_tab, tabs, sc.dc_tab, sc.ac_tab);
  if (t < 64) s_zz[t] = c_dec_zz[t];
  const DecLdsSrc src = dec_stage(s_win, files + sc.data_off, sc.nbytes, (long long)(g - sc.grp0) * DEC_G * (DEC_S / 8));
  __syncthreads();
  if (i >= sc.nsub) return;
  // stores are clamped to the scan's blocks: hd_run stops at blk == nblocks
  uint32_t fl;
  if constexpr (IL) {
    // blk < nblocks keeps base + blk inside the scan's MCUs: the staging array and hd_il_place's grids
    const HdMcu* m = reinterpret_cast<const HdMcu*>(s_mcu);
    HdIlSink sink{m, coeffs + sc.coef_off, dcs + sc.dcs_off, s_zz, (int64_t)sc.blk_base};
    fl = hd_write_lane(src, HdIl{s_tab, m}, entry[slot], (unsigned long long)(i + 1) * DEC_S, (int64_t)blk0[slot],
                       (int64_t)sc.nblocks, i == sc.nsub - 1, sink);
  } else {
    fl = hd_write_lane(src, HdPlain{&s_tab[0], &s_tab[1]}, entry[slot], (unsigned long long)(i + 1) * DEC_S,
                       (int64_t)blk0[slot], (int64_t)sc.nblocks, i == sc.nsub - 1, DecSink{coeffs + sc.coef_off, s_zz});
  }
  if (fl) atomicOr(&status[sc.frame], fl);
}

// DC differences -> values: inclusive sum over the scan's blocks in 64-bit,
// judged against int16 (one 1024-thread workgroup per scan).
__global__ void __launch_bounds__(1024) k_dec_dc(const DecScan* __restrict__ scans, int16_t* __restrict__ coeffs,
                                                 uint32_t* __restrict__ status) {
  __shared__ long long s_w[16];
  const DecScan sc = scans[blockIdx.x];
  if (sc.nblocks == 0) return;
  int16_t* cf = coeffs + sc.coef_off;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long long n = sc.nblocks;
  const long long C = (n + 1023) / 1024, i0 = t * C, i1 = min(n, i0 + C);
  long long loc = 0;
  for (long long i = i0; i < i1; ++i) loc += cf[64 * i];
  long long inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  long long run = inc - loc;
  for (int w = 0; w < wv; ++w) run += s_w[w];
  bool bad = false;
  for (long long i = i0; i < i1; ++i) {
    run += cf[64 * i];
    bad = bad || run < -32768 || run > 32767;
    cf[64 * i] = (int16_t)run;
  }
  if (bad) atomicOr(&status[sc.frame], HD_DC_RANGE);
}

// DC differences of an interleaved scan -> values.  Grid (descriptors, 3): one
// 1024-thread workgroup per descriptor (a scan, or one restart interval of the
// descriptor route: the sum is segmented there) and component.  A component's
// differences are a strided subsequence of the staging array -- hs * vs
// consecutive entries from first[c] in every MCU, padding blocks included --
// summed in scan order with the shape of k_dec_dc; the values of kept blocks
// go to their planar place.
__global__ void __launch_bounds__(1024) k_dec_dc_mcu(const DecScan* __restrict__ scans,
                                                     const HdMcu* __restrict__ mcu, const int16_t* __restrict__ dcs,
                                                     int16_t* __restrict__ coeffs, uint32_t* __restrict__ status) {
  __shared__ long long s_w[16];
  const DecScan sc = scans[blockIdx.x];
  if (sc.nblocks == 0) return;
  const int c = blockIdx.y;  // (uniform: the descriptor's fields below are scalar loads)
  mcu += sc.file;
  dcs += sc.dcs_off;
  const int bpm = mcu->bpm, hs = mcu->hs[c], vs = mcu->vs[c], cnt = hs * vs, first = mcu->first[c];
  const int gw = mcu->gw[c], gh = mcu->gh[c], cols = mcu->mcu_cols;
  int16_t* cf = coeffs + sc.coef_off + mcu->off[c];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const long long n = sc.nblocks / bpm, mcu0 = sc.blk_base / bpm;  // whole MCUs
  const long long C = (n + 1023) / 1024, i0 = t * C, i1 = min(n, i0 + C);
  long long loc = 0;
  for (long long i = i0; i < i1; ++i)
    for (int j = 0; j < cnt; ++j) loc += dcs[(mcu0 + i) * bpm + first + j];
  long long inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  long long run = inc - loc;
  for (int w = 0; w < wv; ++w) run += s_w[w];
  bool bad = false;
  for (long long i = i0; i < i1; ++i) {
    const long long my = (mcu0 + i) / cols, mx = (mcu0 + i) - my * cols;
    for (int j = 0; j < cnt; ++j) {
      run += dcs[(mcu0 + i) * bpm + first + j];
      bad = bad || run < -32768 || run > 32767;
      const long long gx = mx * hs + j % hs, gy = my * vs + j / hs;
      if (gx < gw && gy < gh) cf[64 * (gy * gw + gx)] = (int16_t)run;
    }
  }
  if (bad) atomicOr(&status[sc.frame], HD_DC_RANGE);
}

// ------------------------------------------------------------ driver --

// work: dec_hdr_bytes(n) bytes of device scratch; the scans' (offset, length)
// pairs come first in it (6 n long long).
size_t dec_hdr_bytes(int n) { return sizeof(long long) * 14 * (size_t)n + 4 * (size_t)n; }

hipError_t launch_dec_hdr(const uint8_t* files, long long stride, const unsigned long long* lengths,
                          const uint8_t* hdr_dev, int hl, int n, void* work, uint32_t* status, hipStream_t s) {
  long long* scaninfo = (long long*)work;
  long long* pos = scaninfo + 6 * (size_t)n;
  int* cnt = (int*)(pos + 8 * (size_t)n);
  hipError_t e = hipMemsetAsync(cnt, 0, 4 * (size_t)n, s);
  if (e != hipSuccess) return e;
  const long long per = 256ll * DEC_FIND_B;
  const long long gx = (stride + 16 + per - 1) / per;
  if (gx > 0x7fffffffll || n > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dec_find, dim3((unsigned)gx, n), dim3(256), 0, s, files, stride, lengths, hl, cnt, pos);
  kmark(s, "k_dec_find");
  hipLaunchKernelGGL(k_dec_hdr, dim3(n), dim3(256), 0, s, files, stride, lengths, hdr_dev, hl, cnt, pos, scaninfo,
                     status);
  kmark(s, "k_dec_hdr");
  return hipGetLastError();
}

// The decode of host-described scans, in up to two groups: descriptors of
// interleaved scans and of non-interleaved ones are different instantiations and
// cannot share a launch (a batch of files of both forms has both groups; every
// other caller has one).  A group: nscans entries laid out by dec_layout, ngroups
// workgroups, the longest scan max_ngrp, its own scratch.  Uploads the
// descriptors, zero-fills n_coeffs coefficients, synchronises between
// propagation rounds: the groups' round loops run in step on one `changed`
// counter and one host read per round, so *rounds is the largest any scan of
// either group needs.  A group that has settled early is launched again (its
// workgroups see no changed hand-off and return).  *too_many: the round bound
// was exceeded (a bug, not a property of any input).  status must hold the
// frames' initial words.
hipError_t dec_run_groups(const uint8_t* files, const DecGroup* grp, int ngrp, const HuffDecTab* tabs_dev,
                          int16_t* coeffs, long long n_coeffs, uint32_t* status, hipStream_t s, unsigned* rounds,
                          int* too_many, const HdMcu* mcu_dev, int16_t* dcs) {
  *rounds = 0;
  *too_many = 0;
  hipError_t e = hipMemsetAsync(coeffs, 0, sizeof(int16_t) * (size_t)n_coeffs, s);
  if (e != hipSuccess) return e;
  DecScratch d[2];
  const DecGroup* act[2];
  int na = 0, bound = 0;
  for (int i = 0; i < ngrp && na < 2; ++i)
    if (grp[i].ngroups > 0) {
      d[na] = dec_scratch(grp[i].scratch, grp[i].ngroups, grp[i].nscans);
      bound = grp[i].max_ngrp > bound ? grp[i].max_ngrp : bound;
      act[na++] = &grp[i];
    }
  if (na == 0) return hipSuccess;
  std::vector<int> gs[2];
  for (int a = 0; a < na; ++a) {
    const DecGroup& G = *act[a];
    gs[a].resize((size_t)G.ngroups);
    for (int i = 0; i < G.nscans; ++i)
      for (int g = 0; g < G.sc[i].ngrp; ++g) gs[a][G.sc[i].grp0 + g] = i;
    e = hipMemcpyAsync(d[a].scans, G.sc, sizeof(DecScan) * (size_t)G.nscans, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
      e = hipMemcpyAsync(d[a].grp_scan, gs[a].data(), 4 * (size_t)G.ngroups, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) break;
  }
  const hipError_t e2 = hipStreamSynchronize(s);  // gs is released at return
  if (e != hipSuccess) return e;
  if (e2 != hipSuccess) return e2;
  unsigned* changed = d[0].changed;
  for (int r = 0;; ++r) {
    if (r >= bound) {  // entries of workgroups 0..r are settled after launch r
      *too_many = 1;
      return hipSuccess;
    }
    if ((e = hipMemsetAsync(changed, 0, 4, s)) != hipSuccess) return e;
    for (int a = 0; a < na; ++a) {
      const unsigned grid = (unsigned)act[a]->ngroups;
      if (act[a]->il) {
        hipLaunchKernelGGL(k_dec_sync<true>, dim3(grid), dim3(DEC_G), 0, s, files, d[a].scans, d[a].grp_scan, tabs_dev,
                           d[a].entry, d[a].exitv, d[a].nblk, d[a].gx[(r & 1) ^ 1], d[a].gx[r & 1], changed, r,
                           mcu_dev);
        kmark(s, "k_dec_sync_il");
      } else {
        hipLaunchKernelGGL(k_dec_sync<false>, dim3(grid), dim3(DEC_G), 0, s, files, d[a].scans, d[a].grp_scan,
                           tabs_dev, d[a].entry, d[a].exitv, d[a].nblk, d[a].gx[(r & 1) ^ 1], d[a].gx[r & 1], changed,
                           r, mcu_dev);
        kmark(s, "k_dec_sync");
      }
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    unsigned ch = 0;
    if ((e = hipMemcpyAsync(&ch, changed, 4, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    *rounds = (unsigned)(r + 1);
    if (!ch) break;
  }
  for (int a = 0; a < na; ++a) {
    const DecGroup& G = *act[a];
    const unsigned grid = (unsigned)G.ngroups;
    hipLaunchKernelGGL(k_dec_prefix, dim3(G.nscans), dim3(1024), 0, s, d[a].scans, d[a].nblk, d[a].blk0);
    kmark(s, "k_dec_prefix");
    if (G.il) {  // an interleaved scan's descriptors (the whole scan, or its long restart intervals)
      hipLaunchKernelGGL(k_dec_write<true>, dim3(grid), dim3(DEC_G), 0, s, files, d[a].scans, d[a].grp_scan, tabs_dev,
                         d[a].entry, d[a].blk0, coeffs, status, mcu_dev, dcs);
      kmark(s, "k_dec_write_il");
      if ((e = hipGetLastError()) != hipSuccess) return e;
      hipLaunchKernelGGL(k_dec_dc_mcu, dim3(G.nscans, 3), dim3(1024), 0, s, d[a].scans, mcu_dev, dcs, coeffs, status);
      kmark(s, "k_dec_dc_mcu");
    } else {
      hipLaunchKernelGGL(k_dec_write<false>, dim3(grid), dim3(DEC_G), 0, s, files, d[a].scans, d[a].grp_scan, tabs_dev,
                         d[a].entry, d[a].blk0, coeffs, status, mcu_dev, dcs);
      kmark(s, "k_dec_write");
      if ((e = hipGetLastError()) != hipSuccess) return e;
      hipLaunchKernelGGL(k_dec_dc, dim3(G.nscans), dim3(1024), 0, s, d[a].scans, coeffs, status);
      kmark(s, "k_dec_dc");
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// One group: interleaved when mcu_dev is given.
hipError_t dec_run(const uint8_t* files, const DecScan* sc, int nscans, long long ngroups, int max_ngrp,
                   const HuffDecTab* tabs_dev, void* scratch, int16_t* coeffs, long long n_coeffs, uint32_t* status,
                   hipStream_t s, unsigned* rounds, int* too_many, const HdMcu* mcu_dev, int16_t* dcs) {
  const DecGroup g{sc, nscans, ngroups, max_ngrp, scratch, mcu_dev != nullptr};
  return dec_run_groups(files, &g, 1, tabs_dev, coeffs, n_coeffs, status, s, rounds, too_many, mcu_dev, dcs);
}

// ------------------------------------------------- restart intervals --
//
// A scan with restart intervals (DESIGN.md "Restart intervals") is a row of
// independent streams whose first block is known: one lane per interval
// decodes it once with hd_rst_lane, from state (0, 0) and DC prediction 0.  No
// synchronisation rounds, no block prefix, no scan-wide DC sum, no host read.
//
//   k_rst_scan  plan path, one workgroup per frame: header == the plan's
//               restart header template; marker search (0xFF followed by
//               neither 0x00 nor 0xFF) in file order -- every thread counts
//               the markers of its piece of the file, a prefix over the
//               workgroup turns the counts into ordinals; the list must read
//               SOS, RST0, RST1, .., SOS, .., EOI with the counts the geometry
//               requires; the frame's interval table.
//   k_dec_rst   one lane per interval, 64 intervals per workgroup (one wave).
//
// Byte source of k_dec_rst: bounded global reads through a lane-private LDS
// row (RstRowSrc).  A workgroup's intervals are contiguous in the file but of
// unequal length -- 48 bytes for 64 zero blocks, about 1.2 KB at Q50 noise, about
// 13 KB for 64 blocks of +-1023 -- so a staged window of the whole range fits
// only sometimes; staging it when it fits 32 KiB measured the same as the rows
// alone on all three probe batches and was dropped (DESIGN.md "Restart
// intervals").  Ten global byte loads per symbol, the plain fallback, measured
// 4.8 against 3.4 ms on the Q50 batch.  Reads never leave the interval:
// hd_window masks what lies past its end.
#ifndef JDS_RST_LANE_MAX
#define JDS_RST_LANE_MAX 128  // A/B builds: tools/build_variant.py
#endif
constexpr int RST_LANE_MAX = JDS_RST_LANE_MAX;  // blocks of the longest interval a lane decodes (jds_entropy_restart_info)
constexpr int RST_G = 64;                       // intervals per workgroup: one wave
static_assert(RST_G == 64, "one wave: s_zz is filled by its 64 lanes");

void rst_constants(int* lane_max) { *lane_max = RST_LANE_MAX; }
int rst_group_lanes() { return RST_G; }

// The row holds RST_ROW dwords of the interval from a dword-aligned address on;
// a read outside it refills it (whole dwords inside the interval, single bytes
// at its ragged ends, nothing outside), so a symbol costs LDS reads and a lane
// waits for global memory once per row, not once per symbol.  Rows are
// RST_ROW + 1 dwords apart: lanes reading at the same offset of their rows
// fall on distinct banks.
constexpr int RST_ROW = 32;
struct RstRowSrc {
  uint32_t* row;     // this lane's row
  const uint8_t* d;  // the interval's bytes (global)
  int64_t n;
  int mis;                           // d's misalignment in memory: row dwords are aligned there
  mutable int64_t base = 1ll << 40;  // interval byte of row dword 0 (none yet)
  __device__ __forceinline__ uint32_t byte(int64_t i) const { return d[i]; }
  __device__ __forceinline__ void bytes10(int64_t b, uint64_t& lo, uint64_t& hi) const {
    if (b < base || b + 16 > base + 4 * RST_ROW) {
      base = b - ((b + mis) & 3);
#pragma unroll 8
      for (int q = 0; q < RST_ROW; ++q) {
        const int64_t g = base + 4 * q;
        uint32_t v = 0;
        if (g >= 0 && g + 4 <= n) {
          v = *reinterpret_cast<const uint32_t*>(d + g);
        } else {
          for (int j = 0; j < 4; ++j)
            if (g + j >= 0 && g + j < n) v |= (uint32_t)d[g + j] << (8 * j);
        }
        row[q] = v;
      }
    }
    const int x = (int)(b - base), q = x >> 2, sh = 8 * (x & 3);  // q + 3 < RST_ROW
    const uint64_t a = row[q] | ((uint64_t)row[q + 1] << 32), c = row[q + 2] | ((uint64_t)row[q + 3] << 32);
    lo = sh ? (a >> sh) | (c << (64 - sh)) : a;
    hi = c >> sh;
  }
};

struct DecRstSink {
  int16_t* out;
  const uint8_t* zz;
  int acc;
  bool bad;
  __device__ __forceinline__ void operator()(int64_t blk, int k, int v) {
    if (k == 0) {
      acc += v;
      bad = bad || acc < -32768 || acc > 32767;
      v = acc;
    }
    out[blk * 64 + zz[k]] = (int16_t)v;
  }
};

// IL: an interval is nblk / bpm MCUs of an interleaved scan from scan-order
// block iv.coef_off on; the lane keeps three DC sums (HdIlRstSink).
template <bool IL>
__global__ void __launch_bounds__(RST_G) k_dec_rst(const uint8_t* __restrict__ files, const RstIv* __restrict__ ivs,
                                                   const int niv, const HuffDecTab* __restrict__ tabs,
                                                   int16_t* __restrict__ coeffs, uint32_t* __restrict__ status,
                                                   const HdMcu* __restrict__ mcu) {
  __shared__ HuffDecTab s_tab[4];
  __shared__ __attribute__((aligned(8))) uint32_t s_mcu[IL ? MCU_W : 2];
  __shared__ uint32_t s_row[RST_G * (RST_ROW + 1)];
  __shared__ uint8_t s_zz[64];
  const int t = threadIdx.x;
  const long long i = (long long)blockIdx.x * RST_G + t;
  const int file = ivs[(long long)blockIdx.x * RST_G].file;  // (the grid is ceil(niv / RST_G): inside the list)
  {
    constexpr int NW = (int)(4 * sizeof(HuffDecTab) / 4);
    const uint32_t* a = reinterpret_cast<const uint32_t*>(tabs + 4 * file);
    uint32_t* o = reinterpret_cast<uint32_t*>(s_tab);
    for (int j = t; j < NW; j += RST_G) o[j] = a[j];
  }
  s_zz[t] = c_dec_zz[t];
  if constexpr (IL) {
    const uint32_t* b = reinterpret_cast<const uint32_t*>(mcu + file);
    for (int j = t; j < MCU_W; j += RST_G) s_mcu[j] = b[j];
  }
  RstIv iv{};
  if (i < niv) iv = ivs[i];
  __syncthreads();
  if (iv.nblk <= 0) return;
  const uint8_t* d = files + iv.data_off;
  const RstRowSrc src{s_row + t * (RST_ROW + 1), d, iv.nbytes, (int)((uintptr_t)d & 3u)};
  uint32_t fl;
  bool bad;
  if constexpr (IL) {
    // the host laid the intervals out inside the scan's MCUs: base + blk < its blocks
    const HdMcu* m = reinterpret_cast<const HdMcu*>(s_mcu);
    HdIlRstSink sink{m, coeffs, s_zz, (int64_t)iv.coef_off};
    fl = hd_rst_lane(src, HdIl{s_tab, m}, 0, iv.nblk, sink);
    bad = sink.bad;
  } else {
    DecRstSink sink{coeffs + iv.coef_off, s_zz, 0, false};
    fl = hd_rst_lane(src, HdPlain{&s_tab[iv.tabs & 255], &s_tab[(iv.tabs >> 8) & 255]}, 0, iv.nblk, sink);
    bad = sink.bad;
  }
  if (bad) fl |= HD_DC_RANGE;
  if (fl) atomicOr(&status[iv.frame], fl);
}

// the 16 bytes of the file at [g, g + 16) (g aligned to 16 in memory) that lie in [lo, len): bit j
// of the result is set where byte g + j is a marker's 0xFF
__device__ __forceinline__ uint32_t rst_piece(const uint8_t* __restrict__ d, long long g, long long lo, long long len) {
  if (g + 16 <= lo || g + 1 >= len) return 0u;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (g >= lo && g + 16 <= len) {
    const uint4 v = *reinterpret_cast<const uint4*>(d + g);
    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 16; ++j)
      if (g + j >= lo && g + j < len) w[j >> 2] |= (uint32_t)d[g + j] << (8 * (j & 3));
  }
  bool ff = false;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t x = ~w[k];
    ff = ff || (((x - 0x01010101u) & ~x & 0x80808080u) != 0u);
  }
  if (!ff) return 0u;
  const uint32_t nx = g + 16 < len ? (uint32_t)d[g + 16] : 0u;
  uint32_t m = 0u;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t bj = (w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
    const uint32_t bn = j < 15 ? (w[(j + 1) >> 2] >> (8 * ((j + 1) & 3))) & 0xFFu : nx;
    if (bj == 0xFFu && bn != 0u && bn != 0xFFu && g + j >= lo && g + j + 1 < len) m |= 1u << j;
  }
  return m;
}

// mpos: (first[3] + 1) positions per frame; ivs: first[3] intervals per frame.
__global__ void __launch_bounds__(1024) k_rst_scan(const uint8_t* __restrict__ files, long long stride,
                                                   const unsigned long long* __restrict__ lengths,
                                                   const uint8_t* __restrict__ hdr, int hl, const RstGeo rg,
                                                   long long* __restrict__ mpos, RstIv* __restrict__ ivs,
                                                   uint32_t* __restrict__ status) {
  __shared__ unsigned s_w[16];
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int ni = rg.first[3], nm = ni + 1;  // intervals and markers (3 SOS, the RSTm, EOI) of a frame
  RstIv* iv = ivs + (long long)f * ni;
  long long* mp = mpos + (long long)f * nm;
  const unsigned long long len64 = lengths[f];
  const uint8_t* d = files + (long long)f * stride;
  uint32_t st = 0u;
  if (len64 < (unsigned long long)(hl + 3 * DEC_SOS + 2) || len64 > (unsigned long long)stride) st = HD_BAD_HEADER;  // (uniform)
  const long long len = st ? 0 : (long long)len64;
  if (!st) {
    int bad = 0;
    for (int i = t; i < hl; i += 1024) bad |= d[i] != hdr[(long long)f * hl + i];
    if (__syncthreads_or(bad)) st = HD_BAD_HEADER;
  }
  if (!st) {  // (uniform)
    const long long a0 = hl - (long long)((uintptr_t)(d + hl) & 15u);
    const long long np = (len - a0 + 15) >> 4, C = (np + 1023) / 1024;
    const long long p0 = t * C, p1 = p0 + C < np ? p0 + C : np;
    unsigned loc = 0u;
    for (long long p = p0; p < p1; ++p) loc += (unsigned)__popc(rst_piece(d, a0 + 16 * p, hl, len));
    unsigned inc = loc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned y = __shfl_up(inc, o, 64);
      if (lane >= o) inc += y;
    }
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    unsigned base = 0u, all = 0u;
    for (int w = 0; w < 16; ++w) {
      base += w < wv ? s_w[w] : 0u;
      all += s_w[w];
    }
    if (all != (unsigned)nm) {
      st = HD_RESTART;
    } else {
      unsigned ord = base + inc - loc;
      for (long long p = p0; p < p1 && loc; ++p) {
        uint32_t m = rst_piece(d, a0 + 16 * p, hl, len);
        while (m) {
          const int j = __builtin_ctz(m);
          m &= m - 1u;
          if (ord < (unsigned)nm) mp[ord] = a0 + 16 * p + j;
          ++ord;
        }
      }
      __syncthreads();  // the list (global, this workgroup's writes) is visible
      int bad = 0;
      for (int j = t; j < nm; j += 1024) {
        const long long pos = mp[j];
        if (j == ni) {
          bad |= pos != len - 2 || d[len - 1] != 0xD9;
          continue;
        }
        const int s2 = j < rg.first[1] ? 0 : (j < rg.first[2] ? 1 : 2), k = j - rg.first[s2];
        if (k == 0) {
          const uint8_t sos[DEC_SOS] = {0xFF, 0xDA, 0x00, 0x08, 0x01, (uint8_t)(s2 + 1), (uint8_t)(s2 == 0 ? 0x00 : 0x11),
                                        0x00, 0x3F, 0x00};
          if (pos + DEC_SOS > mp[j + 1] || (j == 0 && pos != hl)) {
            bad = 1;
          } else {
            for (int i = 0; i < DEC_SOS; ++i) bad |= d[pos + i] != sos[i];
          }
        } else {
          bad |= d[pos + 1] != 0xD0 + ((k - 1) & 7);
        }
      }
      if (__syncthreads_or(bad)) st = HD_RESTART;
    }
  }
  for (int j = t; j < ni; j += 1024) {
    const int s2 = j < rg.first[1] ? 0 : (j < rg.first[2] ? 1 : 2), k = j - rg.first[s2];
    RstIv v{};
    v.frame = f;
    v.tabs = s2 ? (1 | (3 << 8)) : (0 | (2 << 8));
    v.coef_off = (long long)f * rg.cpf + rg.off[s2] + 64ll * k * rg.ri;
    if (!st) {
      const long long a = mp[j] + (k == 0 ? DEC_SOS : 2);
      const int rem = rg.nblk[s2] - k * rg.ri;
      v.data_off = (long long)f * stride + a;
      v.nbytes = (int)(mp[j + 1] - a);
      v.nblk = rem < rg.ri ? rem : rg.ri;
    }
    iv[j] = v;
  }
  if (t == 0) status[f] = st;
}

// work of the plan path: the interval table, then the marker list
size_t rst_work_bytes(int n, const RstGeo& rg) {
  return (sizeof(RstIv) * (size_t)rg.first[3] + sizeof(long long) * (size_t)(rg.first[3] + 1)) * (size_t)n;
}

hipError_t launch_dec_rst(const uint8_t* files, const RstIv* ivs_dev, long long niv, const HuffDecTab* tabs_dev,
                          int16_t* coeffs, uint32_t* status, hipStream_t s, const HdMcu* mcu_dev) {
  if (niv <= 0) return hipSuccess;
  if (niv > 0x7fffffffll) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((niv + RST_G - 1) / RST_G));
  if (mcu_dev) {
    hipLaunchKernelGGL(k_dec_rst<true>, grid, dim3(RST_G), 0, s, files, ivs_dev, (int)niv, tabs_dev, coeffs, status,
                       mcu_dev);
    kmark(s, "k_dec_rst_il");
  } else {
    hipLaunchKernelGGL(k_dec_rst<false>, grid, dim3(RST_G), 0, s, files, ivs_dev, (int)niv, tabs_dev, coeffs, status,
                       mcu_dev);
    kmark(s, "k_dec_rst");
  }
  return hipGetLastError();
}

// Plan path: zero-fill, scan every frame's markers, decode every interval.  Enqueues only.
hipError_t launch_dec_rst_plan(const uint8_t* files, long long stride, const unsigned long long* lengths,
                               const uint8_t* hdr_dev, int hl, int n, const RstGeo& rg, void* work,
                               const HuffDecTab* tabs_dev, int16_t* coeffs, uint32_t* status, hipStream_t s) {
  RstIv* ivs = (RstIv*)work;
  long long* mpos = (long long*)(ivs + (size_t)rg.first[3] * (size_t)n);
  hipError_t e = hipMemsetAsync(coeffs, 0, sizeof(int16_t) * (size_t)rg.cpf * (size_t)n, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_rst_scan, dim3(n), dim3(1024), 0, s, files, stride, lengths, hdr_dev, hl, rg, mpos, ivs, status);
  kmark(s, "k_rst_scan");
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return launch_dec_rst(files, ivs, (long long)rg.first[3] * n, tabs_dev, coeffs, status, s, nullptr);
}

}  // namespace jds
