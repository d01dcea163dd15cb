// jds_entropy.hip — baseline JPEG entropy coding of the quantised coefficients
// (SURVEY.md §8(f)4).  The reference stops at a size estimate
// (utils/metrics.py:51-92, "no entropy coding") and keeps the zigzag order
// unused (utils/constants.py:18-27); this turns its all_quantized_coeffs
// (engines/pipeline.py:56,99) into a standard JFIF file per frame: one
// quantisation table (all planes use the luma table, pipeline.py:43), the
// T.81 Annex K standard Huffman tables, three non-interleaved scans (Y, Cb,
// Cr; a non-interleaved scan's raster block order is exactly the reference's
// block order).  Byte-for-byte definition: oracle/jpeg_entropy.py.
//
// Integer / byte work.  Pipeline per batch of frames (segments = 64
// consecutive blocks of one scan, one wave each; DESIGN.md §4 "Round 4: one
// pass"):
//   k_ent_walk   each lane codes its block (zigzag walk, T.81 Annex K tables,
//                left-aligned symbols appended by funnel shifts) into staging
//                words; per-lane bit counts and per-segment totals.
//   k_ent_place  each segment's bit offset within its scan (the sum of the
//                scan's earlier segment totals); each lane's words shifted into place in the packed scan
//                (shared words combined by a segmented OR across the wave,
//                the word shared with the next segment completed from that
//                segment's leading bits), the scan's pad bits, the 0xFF bytes
//                per segment.
//   k_ent_fscan  per frame: 0xFF prefixes, every segment's output offset, the
//                headers (host-built template: SOI, APP0, DQT, SOF0, DHT),
//                the three SOS markers, EOI, file length.
//   k_ent_emit3  stuffed copy to the file (0x00 after every 0xFF).
// With restart interval 64 a segment is a restart interval and one wave codes
// it from start to end: k_rst_code, k_rst_fscan, k_rst_emit (further down).
// The optimised route (jds_encode_jfif_opt, jds_plan_entropy_opt) runs the
// same kernels as OPT = true instantiations behind jds_huffopt.hip's histogram
// and table builder: per-frame tables, headers and header lengths (OptFrame).
// (The rounds 1-3 multi-pass coder -- a counting walk, a block scan, a packing
// walk with LDS atomics, per-chunk stuffing -- measured 0.54 ms per 64 x 1080p
// against this one's 0.30, and a one-launch form with a decoupled look-back
// 0.386 ms; both are retired, their A/Bs are in DESIGN.md §4.)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <initializer_list>

#include "jds_entropy_common.hpp"
#include "jds_entropy_core.hpp"
#include "jds_internal.hpp"

namespace jds {

// ------------------------------------------------------------ tables --

// T.81 Annex K.3 (tables K.3 - K.6): BITS[1..16] and HUFFVAL
static const uint8_t K3_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
static const uint8_t K4_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
static const uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
static const uint8_t K5_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
static const uint8_t K5_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
static const uint8_t K6_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
static const uint8_t K6_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
// utils/constants.py:18-27: row-major index of the k-th zigzag coefficient
static const uint8_t ZZ[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                               12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                               58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Code tables as (length << 16 | code): [0] luma, [1] chroma.
struct EntTab {
  uint32_t dc[2][16];
  uint32_t ac[2][256];
  uint8_t zz[64];
};

// (the left-aligned symbols of the single-pass coder, EsTab: jds_entropy_common.hpp)

// T.81 Annex C: code lengths and codes in order of increasing length
static void huff_codes(const uint8_t* bits, const uint8_t* vals, uint32_t* out, int nsym) {
  for (int i = 0; i < nsym; ++i) out[i] = 0;
  uint32_t code = 0;
  int k = 0;
  for (int len = 1; len <= 16; ++len) {
    for (int i = 0; i < bits[len - 1]; ++i, ++k) out[vals[k]] = ((uint32_t)len << 16) | code++;
    code <<= 1;
  }
}

void ent_build_tables(EntTab* t) {
  memset(t, 0, sizeof *t);
  huff_codes(K3_BITS, DC_VALS, t->dc[0], 16);
  huff_codes(K4_BITS, DC_VALS, t->dc[1], 16);
  huff_codes(K5_BITS, K5_VALS, t->ac[0], 256);
  huff_codes(K6_BITS, K6_VALS, t->ac[1], 256);
  memcpy(t->zz, ZZ, 64);
  // the single-pass coder's left-aligned symbols follow the table (ent_tab_size)
  EsTab* es = reinterpret_cast<EsTab*>(t + 1);
  for (int c = 0; c < 2; ++c) {
    for (int i = 0; i < 16 * ES_RS; ++i) {
      const int run = i / ES_RS, sz = i % ES_RS;
      es->ac[c][i] = sz ? es_left(t->ac[c][(run << 4) | (sz > 10 ? 10 : sz)]) : 0u;
    }
    for (int i = 0; i < 16; ++i) es->dc[c][i] = es_left(t->dc[c][i]);
    es->zrl[c] = es_left(t->ac[c][0xF0]);
    es->eob[c] = es_left(t->ac[c][0x00]);
  }
}

size_t ent_tab_size() { return sizeof(EntTab) + sizeof(EsTab); }
const EsTab* ent_es_tab(const void* tab) { return reinterpret_cast<const EsTab*>((const char*)tab + sizeof(EntTab)); }

// JFIF header template (oracle/jpeg_entropy.py::jfif_headers): returns its length
// (ENT_HDR bytes) or -1 if the table is not baseline (integers in [1, 255]).
int ent_header(const double* q, int mode, int H, int W, uint8_t* o) {
  int p = 0;
  auto put = [&](std::initializer_list<int> b) {
    for (int v : b) o[p++] = (uint8_t)v;
  };
  put({0xFF, 0xD8});
  put({0xFF, 0xE0, 0x00, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  put({0xFF, 0xDB, 0x00, 0x43, 0x00});
  for (int k = 0; k < 64; ++k) {
    const double v = q[ZZ[k]];
    if (!(v >= 1.0 && v <= 255.0) || v != (double)(int)v) return -1;
    o[p++] = (uint8_t)(int)v;
  }
  const int smp = mode == M420 ? 0x22 : (mode == M422 ? 0x21 : 0x11);
  put({0xFF, 0xC0, 0x00, 0x11, 0x08, H >> 8, H & 255, W >> 8, W & 255, 3, 1, smp, 0, 2, 0x11, 0, 3, 0x11, 0});
  const uint8_t* bits[4] = {K3_BITS, K5_BITS, K4_BITS, K6_BITS};
  const uint8_t* vals[4] = {DC_VALS, K5_VALS, DC_VALS, K6_VALS};
  const int nv[4] = {12, 162, 12, 162}, id[4] = {0x00, 0x10, 0x01, 0x11};
  for (int t = 0; t < 4; ++t) {
    const int len = 3 + 16 + nv[t];
    put({0xFF, 0xC4, len >> 8, len & 255, id[t]});
    for (int i = 0; i < 16; ++i) o[p++] = bits[t][i];
    for (int i = 0; i < nv[t]; ++i) o[p++] = vals[t][i];
  }
  return p;
}

// ------------------------------------------------------------ kernels --
// (segment geometry, block registers, wave primitives: jds_entropy_common.hpp)

// ------------------------------------------------ one pass (round 4) --
//
// Segments of 64 consecutive blocks of one scan, one wave each.
//  * walk (k_ent_walk): each lane packs its block MSB-first into lane-private
//    staging words (LDS, word-major across the wave's lanes so every store hits
//    its own bank; words past ES_SW go to the segment's global rows), so the
//    block's bit count comes out of the same walk that packs it.  Appending a
//    symbol is one shift and one OR on a left-aligned 32-bit pending word.
//  * offset: the segment's bit offset within its scan is the sum of the scan's
//    earlier segment totals (k_ent_place sums them itself for short scans, a
//    per-frame prefix launch gives them for long ones).
//  * placement (k_ent_place): each lane writes its words shifted into place.
//    Words it alone covers: plain stores.  A word shared by several lanes is
//    written once, by the lane holding its first bit, with the others' bits
//    gathered by a segmented OR across the wave; the word a segment shares with
//    the next is completed from the next segment's leading bits.
//  * the 0xFF bytes of every word the segment finalises are counted there,
//    and each scan's last byte is padded with 1-bits (T.81 F.1.2.3), so the
//    stuffing pass reads final words.
// A segment that is not the last of its scan holds >= 256 bits (every block
// costs >= 4), so only consecutive segments share a word.  (Optimised tables,
// DESIGN.md "Optimised tables": a block costs >= 2 bits -- a one-symbol DC
// table and a one-symbol AC table have 1-bit codes -- so >= 128 bits per such
// segment, and the same holds.)
//
// OPT (template parameter of the coding kernels): the optimised route.  Its
// code tables, header and header length are per frame (OptFrame, built on the
// device by jds_huffopt.hip); a workgroup's waves can sit in different frames,
// so each wave stages its own frame's table.  The standard route's
// instantiations (OPT = false) carry none of that: one shared table per
// workgroup, the header template's fixed length.
// k_ent_walk packs each segment's blocks and stores the staged words
// (word-major per segment), the lanes' bit counts and the segment's total;
// k_ent_place places the words at the segment's offset.
//
// The code table in LDS (es: [ES_WAVES] on the optimised route, [1] otherwise):
// the standard route stages the one table gt for the workgroup; the optimised
// route has every wave stage its own frame's (a workgroup's segments can span
// frames: three segments per frame at 40 x 72 4:4:4).  Both end in the
// workgroup's barrier, so every wave calls them before it can leave.
__device__ __forceinline__ void es_stage_shared(EsTab* es, const EsTab* __restrict__ gt) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(gt);
  uint32_t* dst = reinterpret_cast<uint32_t*>(es);
  for (int i = threadIdx.x; i < (int)(sizeof(EsTab) / 4); i += blockDim.x) dst[i] = src[i];
  __syncthreads();
}
__device__ __forceinline__ void es_stage_frame(EsTab* es, const OptFrame* __restrict__ of, const EntGeo& e, int g,
                                               int nseg, int lane) {
  const int f = (g < nseg ? g : nseg - 1) / e.sfirst[3];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&of[f].es);
  uint32_t* dst = reinterpret_cast<uint32_t*>(es);
  for (int i = lane; i < (int)(sizeof(EsTab) / 4); i += 64) dst[i] = src[i];
  __syncthreads();
}

template <bool OPT>
__global__ void __launch_bounds__(64 * ES_WAVES) __attribute__((amdgpu_waves_per_eu(ES_WPE))) k_ent_walk(
    const EntGeo e, const int nseg, const int16_t* __restrict__ coeffs, const EsTab* __restrict__ gt,
    uint32_t* __restrict__ gst, uint32_t* __restrict__ nbits, unsigned long long* __restrict__ agg,
    uint32_t* __restrict__ badseg, unsigned long long* __restrict__ ffs, const OptFrame* __restrict__ of) {
  __shared__ EsTab es_s[OPT ? ES_WAVES : 1];
  __shared__ uint32_t stage[ES_WAVES][ES_SW > 0 ? ES_SW : 1][64];
  __shared__ int16_t czs[ES_WAVES][ES_HI > 0 ? ES_HI : 1][64];
  if constexpr (!OPT) es_stage_shared(es_s, gt);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int16_t* cz = &czs[wv][0][lane];
  const int g = blockIdx.x * ES_WAVES + wv;
  if constexpr (OPT) es_stage_frame(&es_s[wv], of, e, g, nseg, lane);
  const EsTab& es = es_s[OPT ? wv : 0];
  if (g >= nseg) return;  // (whole wave; no barrier follows)
  const EsSeg q = es_seg(e, g);
  const int bi = q.seg * 64 + lane;
  const bool valid = bi < q.nbs;
  const long long gb = (long long)q.f * e.nb + e.first[q.s] + (valid ? bi : q.nbs - 1);
  const BlockRegs rg = load_block(coeffs + gb * 64);
  const int dc = coef_at<0>(rg);
  int pred = wave_shr1(dc);
  if (lane == 0) pred = q.seg ? (int)coeffs[(gb - 1) * 64] : 0;
  uint32_t* st = &stage[wv][0][lane];
  uint32_t* ov = gst + (size_t)g * ES_MAXW * 64 + lane;
  uint32_t nb = 0u;
  int k = 0;
  bool bd = false;
  if (valid) {
    EsStage o{st, ov};
    nb = es_block(rg, dc - pred, es, q.s ? 1 : 0, o, bd, cz);
    k = (int)((nb + 31u) >> 5);
  }
  const bool any_bad = __ballot(bd) != 0ull;
  // the LDS slots to the segment's global area (one 256-B row per slot)
  const int kmax = (int)wave_max((uint32_t)(k < ES_SW ? k : ES_SW));
  for (int j = 0; j < kmax; ++j)
    if (j < k) ov[j * 64] = st[j * 64];
  nbits[(size_t)g * 64 + lane] = nb;
  const unsigned long long a = wave_sum(nb);  // (<= 64 * 1660 bits)
  if (lane == 0) {
    agg[g] = a;
    badseg[g] = any_bad ? 1u : 0u;  // not baseline-codable: the frame is reported (k_ent_fscan)
    if (g == nseg - 1) {            // the scans' closing zeros (no memsets)
      agg[nseg] = 0ull;
      ffs[nseg] = 0ull;
    }
  }
}

// The segment's bit offset within its scan is the sum of the scan's earlier
// segment totals.  Scans of at most ES_SELF_MAX segments (1080p: 507 luma, 128
// chroma) sum them here -- every total is final when this launch starts -- and
// need no prefix launch between the walk and the placement (0.245 -> 0.244 ms
// per 64 x 1080p); longer scans (4K: 2025 luma segments) would re-sum O(n^2)
// totals across their waves, so their frames get a per-frame exclusive prefix
// (k_ent_fscan<false>, segoff) before this launch.  Measured
// (tools/ent_probe.py, profiles/r05_entropy_selfpre_ab.jsonl): 16 x 4K, every
// scan summing itself 0.2585 ms, every scan from the prefix launch 0.2517,
// this threshold 0.2547; 64 x 1080p 0.2518 / 0.2523 / 0.2528 (noise).

// incl[g] = the segment's end bit within its scan (k_ent_fscan / k_ent_emit3
// read it as desc)
template <bool OPT>
__global__ void __launch_bounds__(256) k_ent_place(const EntGeo e, const int nseg, const uint32_t* __restrict__ gst,
                                                   const uint32_t* __restrict__ nbits,
                                                   const unsigned long long* __restrict__ agg,
                                                   const unsigned long long* __restrict__ segoff,
                                                   unsigned long long* __restrict__ incl, uint32_t* __restrict__ raw,
                                                   unsigned long long* __restrict__ ffs,
                                                   unsigned long long* __restrict__ info,
                                                   unsigned long long* __restrict__ scan_bits) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= nseg) return;
  const EsSeg q = es_seg(e, g);
  const bool valid = q.seg * 64 + lane < q.nbs;
  const int nvalid = q.nbs - q.seg * 64 < 64 ? q.nbs - q.seg * 64 : 64;
  const bool last_seg = q.seg == q.nseg_s - 1;
  const bool fuse = !last_seg;      // this segment completes the word it shares with the next
  const int gn = fuse ? g + 1 : g;  // the next segment of the scan (its head bits)
  const uint32_t nb = nbits[(size_t)g * 64 + lane];
  const uint32_t nbn = nbits[(size_t)gn * 64 + lane];
  const uint32_t w0n = gst[(size_t)gn * ES_MAXW * 64 + lane];  // (row 0; garbage where nbn == 0)
  unsigned long long pre;
  if (q.nseg_s <= ES_SELF_MAX) {  // (uniform: the scan's length)
    // lane sums are < 2^32 (<= 8 totals of <= 64 * 1660 bits); the wave sum in
    // two DPP scans of 8 / 24 bits
    const unsigned long long* a0 = agg + (g - q.seg);
    uint32_t ps = 0u;
    for (int j0 = 0; j0 < q.seg; j0 += 512) {  // eight loads in flight per lane
      uint32_t t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + 64 * u + lane;
        t[u] = j < q.seg ? (uint32_t)a0[j] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) ps += t[u];
    }
    pre = ((unsigned long long)wave_sum(ps >> 8) << 8) + wave_sum(ps & 255u);
  } else {
    pre = segoff[g] - segoff[g - q.seg];  // (frame-relative prefixes)
  }
  const uint32_t inc = wave_incl_sum(nb, lane), incn = wave_incl_sum(nbn, lane);
  const unsigned long long A = lane63(inc);
  const unsigned long long W1 = pre + A;
  if (lane == 0) incl[g] = W1;
  uint32_t tailx = 0u;
  unsigned long long Wn = 0ull;
  if (fuse) {
    // the next segment's lanes starting inside this segment's final word: each
    // one's bits there are its first staged word's leading bits
    const uint32_t sh = (uint32_t)(W1 & 31ull), p = sh + (incn - nbn);
    tailx = (sh && nbn && p < 32u) ? w0n >> p : 0u;
    tailx = wave_or(tailx);
    const unsigned long long An = lane63(incn);
    if (q.seg + 2 == q.nseg_s && sh && ((W1 + An - 1ull) >> 5) == ((W1 - 1ull) >> 5)) Wn = W1 + An;
  }
  es_place<es_span<OPT>()>(e, q, g, lane, valid, nvalid, last_seg, nb, inc - nb, pre, A, nullptr,
           gst + (size_t)g * ES_MAXW * 64 + lane, (int)((nb + 31u) >> 5), raw, ffs, info, scan_bits, fuse, tailx, Wn,
           raw + raw_base(e, q.f, q.s), true);
}

// One wave per segment: the bytes of the words it finalised, stuffed (0x00
// after every 0xFF) at their place in the file.  Per 1 KiB of input (16 B per
// lane): the lanes' stuffed lengths by a wave prefix, the stuffed bytes
// assembled in the wave's LDS buffer at the output's alignment, then written
// out as aligned dwords (bytes at the two partial ends).
// Per-frame exclusive prefix of a per-segment u64 array (one 1024-thread
// workgroup per frame; frames' segment ranges are independent): out[g] is
// frame-relative, tot[f] the frame's total.  OFFS: also each segment's first
// output byte, from the frame's own prefixes, and the frame's markers.
// (Replaced a hipCUB scan -- two launches -- and a per-segment offset launch.)
// OPT: the frame's header and its length come from its OptFrame.
template <bool OFFS, bool OPT>
__global__ void __launch_bounds__(1024) k_ent_fscan(const EntGeo e, const unsigned long long* __restrict__ in,
                                                    unsigned long long* __restrict__ out,
                                                    unsigned long long* __restrict__ tot,
                                                    const unsigned long long* __restrict__ desc,
                                                    const unsigned long long* __restrict__ info,
                                                    unsigned long long* __restrict__ outoff,
                                                    const uint8_t* __restrict__ hdr, uint8_t* __restrict__ file,
                                                    long long stride, unsigned long long* __restrict__ lengths,
                                                    const uint32_t* __restrict__ badseg,
                                                    const OptFrame* __restrict__ of) {
  __shared__ unsigned long long s_w[16];
  __shared__ int s_bad;
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n = e.sfirst[3];
  const long long g0 = (long long)f * n;
  const int C = (n + 1023) / 1024, i0 = t * C, i1 = min(n, i0 + C);
  unsigned long long loc = 0ull;
  for (int i = i0; i < i1; ++i) loc += in[g0 + i];
  unsigned long long inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  unsigned long long base = 0ull, all = 0ull;
  for (int w = 0; w < 16; ++w) {
    base += w < wv ? s_w[w] : 0ull;
    all += s_w[w];
  }
  unsigned long long run = base + inc - loc;
  for (int i = i0; i < i1; ++i) {
    const unsigned long long v = in[g0 + i];
    out[g0 + i] = run;
    run += v;
  }
  if (t == 0) tot[f] = all;
  if constexpr (OFFS) {
    __syncthreads();  // the frame's prefixes (global, this workgroup's writes) are visible
    const long long hl = OPT ? (long long)of[f].hdr_len : e.hdr;
    const uint8_t* hsrc = OPT ? of[f].hdr : hdr + (long long)f * e.hdr;
    long long so[3];
    long long p = hl + ENT_SOS;
    for (int s2 = 0; s2 < 3; ++s2) {
      so[s2] = p;
      const unsigned long long nb = (info[2 * (f * 3 + s2) + 1] + 7) >> 3;
      const unsigned long long ffe = s2 < 2 ? out[g0 + e.sfirst[s2 + 1]] : all;
      p += (long long)(nb + ffe - out[g0 + e.sfirst[s2]]) + ENT_SOS;
    }
    int b = 0;
    for (int i = t; i < n; i += 1024) {
      const long long g = g0 + i;
      const int s2 = i < e.sfirst[1] ? 0 : (i < e.sfirst[2] ? 1 : 2);
      const int seg = i - e.sfirst[s2];
      const unsigned long long W0 = seg ? desc[g - 1] : 0ull;
      outoff[g] = (unsigned long long)so[s2] + 4 * ((W0 + 31) >> 5) + (out[g] - out[g0 + e.sfirst[s2]]);
      b |= (int)badseg[g];
    }
    // the frame's markers (k_ent_emit3 writes only the scans' bytes)
    if (t == 0) s_bad = 0;
    __syncthreads();
    if (b) s_bad = 1;
    uint8_t* dst = file + (long long)f * stride;
    for (int i = t; i < hl; i += 1024) dst[i] = hsrc[i];
    if (t < 3) {
      uint8_t* m = dst + so[t] - ENT_SOS;
      const uint8_t sos[ENT_SOS] = {0xFF, 0xDA, 0x00, 0x08, 0x01, (uint8_t)(t + 1), (uint8_t)(t == 0 ? 0x00 : 0x11),
                                    0x00, 0x3F, 0x00};
      for (int i = 0; i < ENT_SOS; ++i) m[i] = sos[i];
    }
    __syncthreads();
    if (t == 0) {
      const long long end = p - ENT_SOS;  // end of the Cr scan
      dst[end] = 0xFF;
      dst[end + 1] = 0xD9;
      if (lengths) lengths[f] = s_bad ? 0ull : (unsigned long long)(end + 2);  // 0: not baseline-codable
    }
  }
}

__global__ void __launch_bounds__(256) k_ent_emit3(const EntGeo e, const int nseg,
                                                   const unsigned long long* __restrict__ desc,
                                                   const unsigned long long* __restrict__ info,
                                                   const uint32_t* __restrict__ raw,
                                                   const unsigned long long* __restrict__ outoff,
                                                   uint8_t* __restrict__ out, long long stride) {
  __shared__ uint32_t sbuf[4][(2 * EM_CHUNK + 8) / 4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = blockIdx.x * 4 + wv;
  if (g >= nseg) return;
  const EsSeg q = es_seg(e, g);
  const unsigned long long W0 = q.seg ? desc[g - 1] : 0ull, W1 = desc[g];
  const unsigned long long nbytes = (info[2 * (q.f * 3 + q.s) + 1] + 7) >> 3;
  const unsigned long long fw = (W0 + 31) >> 5, lw = (W1 - 1) >> 5;
  if (fw > lw) return;
  const unsigned long long b0 = 4 * fw, b1 = (4 * lw + 4 < nbytes) ? 4 * lw + 4 : nbytes;
  uint8_t* dst = out + (long long)q.f * stride + (long long)outoff[g];
  const uint32_t* w = raw + raw_base(e, q.f, q.s);
  em_copy(w, b0, b1, dst, sbuf[wv], lane);
}

// ------------------------------------- restart intervals (Ri = 64) --
//
// With a restart interval of 64 blocks a segment IS a restart interval (T.81
// E.1.4; DESIGN.md "Restart intervals"): its first block predicts from 0, it is
// padded to its own byte and nothing of it shares a word with a neighbour.  So
// one wave codes an interval from start to end in one kernel:
//   k_rst_code   walk (es_block) and placement (es_place at bit offset 0 of the
//                segment's own slot, as the last segment of a one-segment scan:
//                pad bits, 0xFF count); the segment's bits.
//   k_rst_fscan  per frame: prefix over the segments' output bytes (data bytes
//                + 0xFF bytes + 2 for the RSTm in front of segments 1.. of a
//                scan) -> every segment's first output byte; the header template
//                (with DRI), the SOS markers, EOI, length, the scans' bits.
//   k_rst_emit   RSTm, then the segment's stuffed bytes.
// A segment's slot is RS_SLOT words of the scan's packed area: 64 blocks of at
// most 1660 bits are exactly 3320 words, so slot seg starts where the plain
// coder's worst case would put block 64 seg, and ent_sizes' areas carry over.
constexpr int RS_INTERVAL = 64;
constexpr int RS_SLOT = 64 * 1660 / 32;
static_assert(RS_SLOT * 32 == 64 * ENT_BLOCK_BITS, "whole words");
// optimised tables: 64 blocks of at most 1665 bits are exactly 3330 words, and
// the packed areas are sized with that bound (ent_geo_opt)
constexpr int RS_SLOT_OPT = 64 * ENT_BLOCK_BITS_OPT / 32;
static_assert(RS_SLOT_OPT * 32 == 64 * ENT_BLOCK_BITS_OPT, "whole words");
template <bool OPT>
constexpr int rs_slot() { return OPT ? RS_SLOT_OPT : RS_SLOT; }
constexpr int RS_DRI = 6;  // FF DD 00 04 Ri(2)

int ent_restart_interval() { return RS_INTERVAL; }

template <bool OPT>
__global__ void __launch_bounds__(64 * ES_WAVES) __attribute__((amdgpu_waves_per_eu(ES_WPE))) k_rst_code(
    const EntGeo e, const int nseg, const int16_t* __restrict__ coeffs, const EsTab* __restrict__ gt,
    uint32_t* gst, uint32_t* __restrict__ raw, unsigned long long* __restrict__ agg, uint32_t* __restrict__ badseg,
    unsigned long long* __restrict__ ffs, const OptFrame* __restrict__ of) {
  __shared__ EsTab es_s[OPT ? ES_WAVES : 1];
  __shared__ uint32_t stage[ES_WAVES][ES_SW > 0 ? ES_SW : 1][64];
  __shared__ int16_t czs[ES_WAVES][ES_HI > 0 ? ES_HI : 1][64];
  if constexpr (!OPT) es_stage_shared(es_s, gt);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int16_t* cz = &czs[wv][0][lane];
  const int g = blockIdx.x * ES_WAVES + wv;
  if constexpr (OPT) es_stage_frame(&es_s[wv], of, e, g, nseg, lane);
  const EsTab& es = es_s[OPT ? wv : 0];
  if (g >= nseg) return;  // (whole wave; no barrier follows)
  const EsSeg q = es_seg(e, g);
  const int bi = q.seg * 64 + lane;
  const bool valid = bi < q.nbs;
  const int nvalid = q.nbs - q.seg * 64 < 64 ? q.nbs - q.seg * 64 : 64;
  const long long gb = (long long)q.f * e.nb + e.first[q.s] + (valid ? bi : q.nbs - 1);
  const BlockRegs rg = load_block(coeffs + gb * 64);
  const int dc = coef_at<0>(rg);
  int pred = wave_shr1(dc);
  if (lane == 0) pred = 0;  // the interval's first block: the prediction restarts
  uint32_t* st = &stage[wv][0][lane];
  uint32_t* ov = gst + (size_t)g * ES_MAXW * 64 + lane;
  uint32_t nb = 0u;
  int k = 0;
  bool bd = false;
  if (valid) {
    EsStage o{st, ov};
    nb = es_block(rg, dc - pred, es, q.s ? 1 : 0, o, bd, cz);
    k = (int)((nb + 31u) >> 5);
  }
  const bool any_bad = __ballot(bd) != 0ull;
  const uint32_t inc = wave_incl_sum(nb, lane);
  const unsigned long long A = lane63(inc);  // (<= 64 * 1660 bits)
  // the lane reads back its own staged words: LDS slots and, past ES_SW, its own global stores
  es_place<es_span<OPT>()>(e, q, g, lane, valid, nvalid, true, nb, inc - nb, 0ull, A, st, ov, k, raw, ffs, nullptr,
                           nullptr, false, 0u, 0ull,
                           raw + raw_base(e, q.f, q.s) + (long long)q.seg * rs_slot<OPT>(), false);
  if (lane == 0) {
    agg[g] = A;
    badseg[g] = any_bad ? 1u : 0u;
  }
}

template <bool OPT>
__global__ void __launch_bounds__(1024) k_rst_fscan(const EntGeo e, const unsigned long long* __restrict__ agg,
                                                    const unsigned long long* __restrict__ ffs,
                                                    unsigned long long* __restrict__ outoff,
                                                    const uint8_t* __restrict__ hdr, uint8_t* __restrict__ file,
                                                    long long stride, unsigned long long* __restrict__ lengths,
                                                    unsigned long long* __restrict__ scan_bits,
                                                    const uint32_t* __restrict__ badseg,
                                                    const OptFrame* __restrict__ of) {
  __shared__ unsigned long long s_w[16], s_bits[3], s_first[3];
  __shared__ int s_bad;
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int n = e.sfirst[3];
  const long long g0 = (long long)f * n;
  const long long h0 = OPT ? (long long)of[f].hdr_len : e.hdr;  // the header before DRI
  const uint8_t* hsrc = OPT ? of[f].hdr : hdr + (long long)f * e.hdr;
  const long long hl = h0 + RS_DRI;
  if (t < 3) s_bits[t] = 0ull;
  if (t == 0) s_bad = 0;
  __syncthreads();
  auto scan_of = [&](int i) { return i < e.sfirst[1] ? 0 : (i < e.sfirst[2] ? 1 : 2); };
  auto bytes_of = [&](int i) {  // the segment's output bytes, its RSTm included
    return ((agg[g0 + i] + 7) >> 3) + ffs[g0 + i] + (i != e.sfirst[scan_of(i)] ? 2ull : 0ull);
  };
  const int C = (n + 1023) / 1024, i0 = t * C, i1 = min(n, i0 + C);
  unsigned long long loc = 0ull, bits[3] = {0ull, 0ull, 0ull};
  int b = 0;
  for (int i = i0; i < i1; ++i) {
    loc += bytes_of(i);
    bits[scan_of(i)] += agg[g0 + i];
    b |= (int)badseg[g0 + i];
  }
  for (int s2 = 0; s2 < 3; ++s2)
    if (bits[s2]) atomicAdd(&s_bits[s2], bits[s2]);
  if (b) s_bad = 1;
  unsigned long long inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  unsigned long long base = 0ull, all = 0ull;
  for (int w = 0; w < 16; ++w) {
    base += w < wv ? s_w[w] : 0ull;
    all += s_w[w];
  }
  unsigned long long run = base + inc - loc;
  for (int i = i0; i < i1; ++i) {
    const int s2 = scan_of(i);
    // the frame's bytes before this segment: header, the SOS of scans 0..s2, the earlier segments
    outoff[g0 + i] = (unsigned long long)(hl + ENT_SOS * (s2 + 1)) + run;
    if (i == e.sfirst[s2]) s_first[s2] = run;
    run += bytes_of(i);
  }
  uint8_t* dst = file + (long long)f * stride;
  for (int i = t; i < h0; i += 1024) dst[i] = hsrc[i];
  if (t == 0) {
    const uint8_t dri[RS_DRI] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(RS_INTERVAL >> 8), (uint8_t)(RS_INTERVAL & 255)};
    for (int i = 0; i < RS_DRI; ++i) dst[h0 + i] = dri[i];
  }
  __syncthreads();
  if (t < 3) {
    uint8_t* m = dst + hl + ENT_SOS * t + (long long)s_first[t];
    const uint8_t sos[ENT_SOS] = {0xFF, 0xDA, 0x00, 0x08, 0x01, (uint8_t)(t + 1), (uint8_t)(t == 0 ? 0x00 : 0x11),
                                  0x00, 0x3F, 0x00};
    for (int i = 0; i < ENT_SOS; ++i) m[i] = sos[i];
    if (scan_bits) scan_bits[f * 3 + t] = s_bits[t];
  }
  if (t == 0) {
    const long long end = hl + 3 * ENT_SOS + (long long)all;
    dst[end] = 0xFF;
    dst[end + 1] = 0xD9;
    if (lengths) lengths[f] = s_bad ? 0ull : (unsigned long long)(end + 2);  // 0: not baseline-codable
  }
}

template <bool OPT>
__global__ void __launch_bounds__(256) k_rst_emit(const EntGeo e, const int nseg,
                                                  const unsigned long long* __restrict__ agg,
                                                  const uint32_t* __restrict__ raw,
                                                  const unsigned long long* __restrict__ outoff,
                                                  uint8_t* __restrict__ out, long long stride) {
  __shared__ uint32_t sbuf[4][(2 * EM_CHUNK + 8) / 4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = blockIdx.x * 4 + wv;
  if (g >= nseg) return;
  const EsSeg q = es_seg(e, g);
  uint8_t* dst = out + (long long)q.f * stride + (long long)outoff[g];
  if (q.seg) {
    if (lane == 0) {
      dst[0] = 0xFF;
      dst[1] = (uint8_t)(0xD0 + ((q.seg - 1) & 7));
    }
    dst += 2;
  }
  em_copy(raw + raw_base(e, q.f, q.s) + (long long)q.seg * rs_slot<OPT>(), 0ull, (agg[g] + 7) >> 3, dst, sbuf[wv],
          lane);
}

// ------------------------------------------------------------ driver --

// Capacity derivation.  A block's worst case is ENT_BLOCK_BITS (1660 >= 1658:
// DC 9 + 11 bits, 63 x (16 + 10) AC) with the Annex K tables and
// ENT_BLOCK_BITS_OPT (1665: DC 16 + 11, 63 x (16 + 10)) with optimised ones,
// where any symbol may get a 16-bit code.  cap_w[s] = the scan's blocks at that
// bound, in words, + 2; a restart interval's slot is 64 blocks at the bound
// (RS_SLOT / RS_SLOT_OPT); a block's staged words ES_MAXW = 53 cover both.  The
// optimised headers are never longer than the template (at most 12 DC and 162
// AC symbols: the histogram clamps like the coder), so the file bounds differ
// only through cap_w: ent_capacity_opt > ent_capacity, and the optimised route
// has its own capacity call while the existing calls keep their values.
static EntGeo ent_geo_bits(const Geo& g, int block_bits) {
  EntGeo e{};
  const int ny = g.nby * g.nbx, nc = g.ncy * g.ncx;
  e.nb = ny + 2 * nc;
  e.first[0] = 0;
  e.first[1] = ny;
  e.first[2] = ny + nc;
  e.first[3] = e.nb;
  e.sfirst[0] = 0;
  for (int s = 0; s < 3; ++s) e.sfirst[s + 1] = e.sfirst[s] + (e.first[s + 1] - e.first[s] + 63) / 64;
  e.cap_w[0] = (int)(((long long)ny * block_bits + 31) / 32) + 2;
  e.cap_w[1] = e.cap_w[2] = (int)(((long long)nc * block_bits + 31) / 32) + 2;
  e.raw_w = (long long)e.cap_w[0] + 2LL * e.cap_w[1];
  e.hdr = ENT_HDR;
  return e;
}

EntGeo ent_geo(const Geo& g) { return ent_geo_bits(g, ENT_BLOCK_BITS); }
EntGeo ent_geo_opt(const Geo& g) { return ent_geo_bits(g, ENT_BLOCK_BITS_OPT); }

// worst case file: header + 3 SOS + every scan at 1660 bits per block, all bytes stuffed + EOI
long long ent_capacity(const Geo& g) {
  const EntGeo e = ent_geo(g);
  return e.hdr + 3 * ENT_SOS + 2 * 4 * e.raw_w + 2;
}

// the same at 1665 bits per block; restart files: + DRI and 4 bytes per interval (ent_capacity_rst)
long long ent_capacity_opt(const Geo& g, bool rst) {
  const EntGeo e = ent_geo_opt(g);
  return e.hdr + 3 * ENT_SOS + 2 * 4 * e.raw_w + 2 + (rst ? 6 + 4ll * e.sfirst[3] : 0);
}

// scratch sizes (bytes): [0] segment end bits (desc, from the second word),
// segment totals (agg; reused for the output offsets once placed), their
// per-frame prefix (segoff), per-lane bit counts, per-segment error flags; [1]
// staged words (word-major per segment); [2] info; [3] packed scans; [4] 0xFF
// counts per segment; [5] their prefix and the frame totals; [6] headers; [7]
// the optimised route's per-frame state (OptFrame).  The packed scans are
// sized for the optimised route's bound, which covers the standard one.
void ent_sizes(const Geo& g, int n, size_t* sz) {
  const EntGeo e = ent_geo_opt(g);
  sz[2] = sizeof(unsigned long long) * 7 * n;  // 6 per frame (scan start / bits) + the frame's error flag
  sz[3] = sizeof(uint32_t) * e.raw_w * n;
  sz[6] = (size_t)e.hdr * n;
  const long long nseg = (long long)n * e.sfirst[3];
  sz[0] = sizeof(unsigned long long) * (nseg + 2) + sizeof(unsigned long long) * 2 * (nseg + 1) +
          sizeof(uint32_t) * 65 * nseg;
  sz[1] = sizeof(uint32_t) * ES_MAXW * 64 * nseg;
  sz[4] = sizeof(unsigned long long) * (nseg + 1);
  sz[5] = sizeof(unsigned long long) * (nseg + 1 + n);  // + the frame totals (k_ent_fscan)
  sz[7] = sizeof(OptFrame) * (size_t)n;
}

// The optimised route's front: zeroed counters, the symbol histogram, the
// frames' tables and headers (jds_huffopt.hip) -- all on the stream, no host
// read between the histogram and the file.
static hipError_t launch_opt_front(const EntGeo& e, int n, int nseg, const int16_t* coeffs, bool rst,
                                   const uint8_t* hdr_dev, const EsTab* est, OptFrame* of, hipStream_t s) {
  hipError_t err = hipMemsetAsync(of, 0, sizeof(OptFrame) * (size_t)n, s);
  if (err != hipSuccess) return err;
  if ((err = launch_ent_hist(e, nseg, coeffs, rst, of, s)) != hipSuccess) return err;
  return launch_opt_tables(n, est, hdr_dev, e.hdr, of, s);
}

// walk, (per-frame segment prefix for long scans,) placement, per-frame
// offsets and markers, stuffing: 4 or 5 launches per batch of frames
// (OPT: after launch_opt_front's three)
template <bool OPT>
static hipError_t launch_entropy_fused(const Geo& g, int n, const int16_t* coeffs, void* const* buf,
                                       const uint8_t* hdr_dev, const void* tab_dev, uint8_t* out, long long stride,
                                       unsigned long long* lengths, unsigned long long* scan_bits, hipStream_t s) {
  const EntGeo e = OPT ? ent_geo_opt(g) : ent_geo(g);
  const long long nseg_l = (long long)n * e.sfirst[3];
  if (nseg_l >= (1ll << 31)) return hipErrorInvalidValue;
  const int nseg = (int)nseg_l;
  auto* desc = (unsigned long long*)buf[0] + 1;
  auto* agg = desc + nseg + 1;
  auto* segoff = agg + nseg + 1;
  auto* nbits = (uint32_t*)(segoff + nseg + 1);
  auto* badseg = nbits + 64 * (size_t)nseg;
  auto* outoff = agg;  // (the segment totals, consumed by the placement)
  auto* ovf = (uint32_t*)buf[1];
  auto* info = (unsigned long long*)buf[2];
  auto* raw = (uint32_t*)buf[3];
  auto* ffs = (unsigned long long*)buf[4];
  auto* ffx = (unsigned long long*)buf[5];
  OptFrame* of = OPT ? (OptFrame*)buf[7] : nullptr;
  const unsigned wg = (unsigned)((nseg + ES_WAVES - 1) / ES_WAVES);
  const unsigned wg4 = (unsigned)((nseg + 3) / 4);  // k_ent_place / k_ent_emit3: four segment waves per workgroup
  const EsTab* est = reinterpret_cast<const EsTab*>((const char*)tab_dev + sizeof(EntTab));
  hipError_t err;
  if constexpr (OPT) {
    if ((err = launch_opt_front(e, n, nseg, coeffs, false, hdr_dev, est, of, s)) != hipSuccess) return err;
  }
  hipLaunchKernelGGL(k_ent_walk<OPT>, dim3(wg), dim3(64 * ES_WAVES), 0, s, e, nseg, coeffs, est, ovf, nbits, agg,
                     badseg, ffs, of);
  kmark(s, OPT ? "k_ent_walk<opt>" : "k_ent_walk");
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  bool long_scan = false;
  for (int c = 0; c < 3; ++c) long_scan = long_scan || e.sfirst[c + 1] - e.sfirst[c] > ES_SELF_MAX;
  if (long_scan) {
    hipLaunchKernelGGL((k_ent_fscan<false, false>), dim3(n), dim3(1024), 0, s, e, agg, segoff, ffx, nullptr, nullptr,
                       nullptr, nullptr, nullptr, 0ll, nullptr, nullptr, nullptr);
    kmark(s, "k_ent_fscan<0>");
  }
  hipLaunchKernelGGL(k_ent_place<OPT>, dim3(wg4), dim3(256), 0, s, e, nseg, ovf, nbits, agg, segoff, desc, raw, ffs,
                     info, scan_bits);
  kmark(s, OPT ? "k_ent_place<opt>" : "k_ent_place");
  if ((err = hipGetLastError()) != hipSuccess) return err;
  // frame-relative 0xFF prefixes, each segment's output offset and the frame's
  // markers in one launch; frame totals in ffx[nseg + 1 ..]
  unsigned long long* fftot = ffx + nseg + 1;
  hipLaunchKernelGGL((k_ent_fscan<true, OPT>), dim3(n), dim3(1024), 0, s, e, ffs, ffx, fftot, desc, info, outoff,
                     hdr_dev, out, stride, lengths, badseg, of);
  kmark(s, OPT ? "k_ent_fscan<1,opt>" : "k_ent_fscan<1>");
  hipLaunchKernelGGL(k_ent_emit3, dim3(wg4), dim3(256), 0, s, e, nseg, desc, info, raw, outoff, out, stride);
  kmark(s, "k_ent_emit3");
  return hipGetLastError();
}

hipError_t launch_entropy(const Geo& g, int n, const int16_t* coeffs, void* const* buf, const uint8_t* hdr_dev,
                          const void* tab_dev, uint8_t* out, long long stride, unsigned long long* lengths,
                          unsigned long long* scan_bits, hipStream_t s) {
  return launch_entropy_fused<false>(g, n, coeffs, buf, hdr_dev, tab_dev, out, stride, lengths, scan_bits, s);
}

hipError_t launch_entropy_opt(const Geo& g, int n, const int16_t* coeffs, void* const* buf, const uint8_t* hdr_dev,
                              const void* tab_dev, uint8_t* out, long long stride, unsigned long long* lengths,
                              unsigned long long* scan_bits, hipStream_t s) {
  return launch_entropy_fused<true>(g, n, coeffs, buf, hdr_dev, tab_dev, out, stride, lengths, scan_bits, s);
}

// The restart header template: the plain one, then DRI.  Returns its length or -1.
int ent_header_rst(const double* q, int mode, int H, int W, int interval, uint8_t* o) {
  const int p = ent_header(q, mode, H, W, o);
  if (p < 0) return -1;
  const uint8_t dri[RS_DRI] = {0xFF, 0xDD, 0x00, 0x04, (uint8_t)(interval >> 8), (uint8_t)(interval & 255)};
  memcpy(o + p, dri, RS_DRI);
  return p + RS_DRI;
}

// Worst-case restart file: the plain bound (header, 3 SOS, every scan at 1660
// bits per block with all bytes stuffed, EOI) + the DRI segment + per interval
// its 2 marker bytes and the pad byte its own byte boundary can add beyond the
// scan's single one -- which, all pad bits being 1, can itself be an 0xFF with
// its stuffed 0x00: 4 bytes per interval.
long long ent_capacity_rst(const Geo& g) {
  const EntGeo e = ent_geo(g);
  return ent_capacity(g) + RS_DRI + 4ll * e.sfirst[3];
}
static_assert(RS_DRI == 6, "ent_capacity_opt's DRI bytes");

// code + place, per-frame offsets and markers, stuffing: 3 launches per batch of
// frames, scratch as launch_entropy's (ent_sizes)
template <bool OPT>
static hipError_t launch_entropy_rst_t(const Geo& g, int n, const int16_t* coeffs, void* const* buf,
                                       const uint8_t* hdr_dev, const void* tab_dev, uint8_t* out, long long stride,
                                       unsigned long long* lengths, unsigned long long* scan_bits, hipStream_t s) {
  const EntGeo e = OPT ? ent_geo_opt(g) : ent_geo(g);
  const long long nseg_l = (long long)n * e.sfirst[3];
  if (nseg_l >= (1ll << 31)) return hipErrorInvalidValue;
  const int nseg = (int)nseg_l;
  auto* desc = (unsigned long long*)buf[0] + 1;
  auto* agg = desc + nseg + 1;
  auto* outoff = agg + nseg + 1;  // (the plain path's segoff)
  auto* badseg = (uint32_t*)(outoff + nseg + 1) + 64 * (size_t)nseg;
  auto* ovf = (uint32_t*)buf[1];
  auto* raw = (uint32_t*)buf[3];
  auto* ffs = (unsigned long long*)buf[4];
  OptFrame* of = OPT ? (OptFrame*)buf[7] : nullptr;
  const unsigned wg = (unsigned)((nseg + ES_WAVES - 1) / ES_WAVES);
  const unsigned wg4 = (unsigned)((nseg + 3) / 4);
  const EsTab* est = reinterpret_cast<const EsTab*>((const char*)tab_dev + sizeof(EntTab));
  hipError_t err;
  if constexpr (OPT) {
    if ((err = launch_opt_front(e, n, nseg, coeffs, true, hdr_dev, est, of, s)) != hipSuccess) return err;
  }
  hipLaunchKernelGGL(k_rst_code<OPT>, dim3(wg), dim3(64 * ES_WAVES), 0, s, e, nseg, coeffs, est, ovf, raw, agg,
                     badseg, ffs, of);
  kmark(s, OPT ? "k_rst_code<opt>" : "k_rst_code");
  err = hipGetLastError();
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(k_rst_fscan<OPT>, dim3(n), dim3(1024), 0, s, e, agg, ffs, outoff, hdr_dev, out, stride, lengths,
                     scan_bits, badseg, of);
  kmark(s, OPT ? "k_rst_fscan<opt>" : "k_rst_fscan");
  hipLaunchKernelGGL(k_rst_emit<OPT>, dim3(wg4), dim3(256), 0, s, e, nseg, agg, raw, outoff, out, stride);
  kmark(s, OPT ? "k_rst_emit<opt>" : "k_rst_emit");
  return hipGetLastError();
}

hipError_t launch_entropy_rst(const Geo& g, int n, const int16_t* coeffs, void* const* buf, const uint8_t* hdr_dev,
                              const void* tab_dev, uint8_t* out, long long stride, unsigned long long* lengths,
                              unsigned long long* scan_bits, hipStream_t s) {
  return launch_entropy_rst_t<false>(g, n, coeffs, buf, hdr_dev, tab_dev, out, stride, lengths, scan_bits, s);
}

hipError_t launch_entropy_rst_opt(const Geo& g, int n, const int16_t* coeffs, void* const* buf,
                                  const uint8_t* hdr_dev, const void* tab_dev, uint8_t* out, long long stride,
                                  unsigned long long* lengths, unsigned long long* scan_bits, hipStream_t s) {
  return launch_entropy_rst_t<true>(g, n, coeffs, buf, hdr_dev, tab_dev, out, stride, lengths, scan_bits, s);
}

// The Annex K table idx (0 DC luma, 1 AC luma, 2 DC chroma, 3 AC chroma): what
// a table class falls back to (jds_selftest_huffopt).
int ent_std_table(int idx, const uint8_t** bits, const uint8_t** vals) {
  const uint8_t* b[4] = {K3_BITS, K5_BITS, K4_BITS, K6_BITS};
  const uint8_t* v[4] = {DC_VALS, K5_VALS, DC_VALS, K6_VALS};
  *bits = b[idx & 3];
  *vals = v[idx & 3];
  return (idx & 1) ? 162 : 12;
}

}  // namespace jds

