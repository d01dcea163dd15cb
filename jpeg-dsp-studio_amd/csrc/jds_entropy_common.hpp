// jds_entropy_common.hpp — what the entropy coder's translation units share
// (jds_entropy.hip: the coding kernels; jds_huffopt.hip: the symbol histogram
// and the table builder of the optimised route): the left-aligned symbol
// table, the segment geometry, the block registers and the wave primitives.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace jds {

// left-aligned symbols: code << (32 - len) | len (len <= 16 sits below the code)
// AC table row stride: (run, size) at run * 11 + size spreads a wave's lookups
// over the LDS banks (32: 0.271 vs 11: 0.258 ms per 64 x 1080p; a stride of 32
// put every even run on the same 11 banks)
constexpr int ES_RS = 11;
static_assert(ES_RS >= 11, "sizes 0..10");
struct EsTab {
  uint32_t ac[2][16 * ES_RS];  // (run & 15, size) -> AC symbol, size clamped to 10 (code_ac's clamp); 0 for size 0
  uint32_t dc[2][16];
  uint32_t zrl[2], eob[2];
};

__host__ __device__ __forceinline__ uint32_t es_left(uint32_t e) {  // (len << 16 | code) -> left-aligned | len
  const uint32_t len = e >> 16;
  return len ? (((e & 0xFFFFu) << (32u - len)) | len) : 0u;
}

// Worst-case bits of one block.  Annex K tables: DC 9 + 11, 63 x (16 + 10) AC =
// 1658, rounded to 1660.  An optimised table may give ANY symbol a 16-bit code:
// DC 16 + 11 and 63 x (16 + 10) = 1665 (no EOB when coefficient 63 is set, and
// ZRLs only replace coefficients that would cost more).
constexpr int ENT_BLOCK_BITS = 1660;
constexpr int ENT_BLOCK_BITS_OPT = 1665;

struct EntGeo {
  int nb;          // blocks per frame (Y + Cb + Cr)
  int first[4];    // first block of each scan within the frame, first[3] = nb
  int sfirst[4];   // single-pass coder: first 64-block segment of each scan within the frame, sfirst[3] = per frame
  int cap_w[3];    // packed-scan capacity in 32-bit words (worst case ENT_BLOCK_BITS[_OPT] per block)
  long long raw_w; // packed words per frame
  long long hdr;   // header template bytes per frame
};

__device__ __forceinline__ long long raw_base(const EntGeo& e, int frame, int s) {
  return (long long)frame * e.raw_w + (s == 0 ? 0 : (s == 1 ? e.cap_w[0] : e.cap_w[0] + e.cap_w[1]));
}

// Inclusive prefix sum over the wave (every lane active): row_shr 1, 2, 4, 8
// within the 16-lane rows, then row_bcast 15 / 31 across them -- six DPP adds
// (the log-step shuffle form, six ds_bpermute round trips, measured slower).
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v, int lane) {
  (void)lane;
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
  v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
  return v;
}

__device__ __forceinline__ int wave_excl_sum(int x, int lane) {
  return (int)(wave_incl_sum((uint32_t)x, lane) - (uint32_t)x);
}

__device__ __forceinline__ uint32_t lane63(uint32_t v) { return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }

// lane l <- lane l + 1 across the whole wave (DPP wave_shl:1; lane 63 <- 0)
__device__ __forceinline__ uint32_t wave_shl1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x130, 0xf, 0xf, true);
}
// lane l <- lane l - 1 (DPP wave_shr:1; lane 0 <- 0)
__device__ __forceinline__ int wave_shr1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x138, 0xf, 0xf, true); }

// wave-wide totals (every lane active), read from lane 63 of the DPP scan
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) { return lane63(wave_incl_sum(v, (int)__lane_id())); }

__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false);
  v |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false);
  return lane63(v);
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, false));
  v = max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, false));
  return lane63(v);
}

// One LANE per block: its 64 coefficients sit in 32 VGPRs (packed int16
// pairs) and the zigzag walk is unrolled at compile time, so every register
// index is a constant; the per-coefficient work is a handful of integer ops
// under the lane's own "nonzero" mask.  (A wave per block, one lane per
// coefficient, spent ~400 wave instructions per block on ballots, shuffles
// and divergent branches.)
struct BlockRegs {
  uint32_t w[32];
};

__device__ __forceinline__ BlockRegs load_block(const int16_t* __restrict__ p) {
  BlockRegs r;
  const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint4 x = q[i];
    r.w[4 * i] = x.x; r.w[4 * i + 1] = x.y; r.w[4 * i + 2] = x.z; r.w[4 * i + 3] = x.w;
  }
  return r;
}

template <int IDX>
__device__ __forceinline__ int coef_at(const BlockRegs& r) {
  return (int)(int16_t)((IDX & 1) ? (r.w[IDX >> 1] >> 16) : (r.w[IDX >> 1] & 0xFFFFu));
}

constexpr uint8_t ZZC[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                             12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                             58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// size category of |v| (clamped to 10, code_ac's clamp)
__device__ __forceinline__ int es_size(int a) {
  const int sz = a ? 32 - __clz(a) : 0;
  return sz > 10 ? 10 : sz;
}

struct EsSeg {
  int f, s, seg, nseg_s, nbs;
};
__device__ __forceinline__ EsSeg es_seg(const EntGeo& e, int g) {
  EsSeg q;
  q.f = g / e.sfirst[3];
  const int r = g - q.f * e.sfirst[3];
  q.s = r < e.sfirst[1] ? 0 : (r < e.sfirst[2] ? 1 : 2);
  q.seg = r - e.sfirst[q.s];
  q.nseg_s = e.sfirst[q.s + 1] - e.sfirst[q.s];
  q.nbs = e.first[q.s + 1] - e.first[q.s];
  return q;
}

// The JFIF header template: SOI APP0 DQT SOF0, then the four DHT segments
// (0x00, 0x10, 0x01, 0x11: 12, 162, 12, 162 values in the Annex K tables)
constexpr int ENT_HDR_FIXED = 2 + 18 + 69 + 19;
constexpr int ENT_DHT_HEAD = 4 + 1 + 16;  // marker, length, Tc/Th, BITS
constexpr int ENT_HDR = ENT_HDR_FIXED + 2 * (ENT_DHT_HEAD + 12) + 2 * (ENT_DHT_HEAD + 162);
constexpr int ENT_SOS = 10;

// The optimised route's per-frame state (k_ent_hist counts, k_ent_opt_tables
// builds, the coding kernels read): all of one frame in one OptFrame.
constexpr int OPT_BINS = 16 + 256;  // DC categories, AC symbols
struct OptFrame {
  uint32_t cnt[2][OPT_BINS];   // [luma / chroma][DC 0..15, AC 0..255]
  EsTab es;                    // the frame's code tables
  uint32_t hdr_len;            // the frame's header bytes (<= ENT_HDR)
  uint32_t pad_[3];
  uint8_t hdr[(ENT_HDR + 15) / 16 * 16];  // SOI .. the fourth DHT
};
static_assert(sizeof(OptFrame) % 16 == 0, "frames stay 16-byte aligned");

// jds_huffopt.hip.  launch_ent_hist: the symbol counts of nseg segments into
// of[frame].cnt (zeroed by the caller); rst: DC prediction restarts at every
// segment.  launch_opt_tables: of[f].es / hdr / hdr_len from of[f].cnt, the
// fixed header bytes and any fallback table from the frame's header template
// (hdr_std + f * hdr_stride) and the Annex K symbol table std_tab.
hipError_t launch_ent_hist(const EntGeo& e, int nseg, const int16_t* coeffs, bool rst, OptFrame* of, hipStream_t s);
hipError_t launch_opt_tables(int n, const EsTab* std_tab, const uint8_t* hdr_std, long long hdr_stride, OptFrame* of,
                             hipStream_t s);

}  // namespace jds
