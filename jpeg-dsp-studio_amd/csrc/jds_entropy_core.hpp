// jds_entropy_core.hpp — the device cores of the one-pass entropy coder that
// its translation units share (jds_entropy.hip: the three-scan writer;
// jds_entropy_mcu.hip: the interleaved-scan writer): the staged block walk
// (es_block), the placement of a segment's staged words (es_place) and the
// stuffed copy (em_copy).  What they do and why is told where the pipeline is:
// jds_entropy.hip, "one pass (round 4)".  Every function is inlined into the
// kernels of the unit that includes this; no device code crosses units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_entropy_common.hpp"

namespace jds {

constexpr int ES_WPE = 4;     // waves per SIMD the walk's registers are held to (3..6: no difference)
constexpr int ES_DENSE = 32;  // zigzag positions coded by the unrolled walk; the rest by the nonzero loop
// LDS staging words per lane (more go to global): 16: 0.303, 0: 0.295, 8: 0.292
// ms per 64 x 1080p (LDS -> 5 workgroups per CU)
constexpr int ES_SW = 8;
constexpr int ES_HI = 64 - ES_DENSE;     // positions of the nonzero loop
static_assert(ES_HI <= 32, "es_hi_stash's nonzero mask is one 32-bit word (ES_DENSE = 24 dropped positions 56-63)");
// words per block at most: the spill area.  1660 bits (Annex K tables) and 1665
// (optimised tables, ENT_BLOCK_BITS_OPT) both end in word 53 (52 * 32 = 1664)
constexpr int ES_MAXW = 53;
static_assert(32 * ES_MAXW >= ENT_BLOCK_BITS_OPT && ENT_BLOCK_BITS_OPT >= ENT_BLOCK_BITS, "a block's staged words");
// lanes one 32-bit word can hold whole, + 1: the reach of es_place's segmented
// OR.  Every block costs >= 4 bits with the Annex K tables (7 whole blocks
// between a tail bit and a head bit), >= 2 with optimised ones (15).
template <bool OPT>
constexpr int es_span() { return OPT ? 15 : 7; }
#ifndef JDS_ES_WAVES  // tools: A/B builds of the walk's waves per workgroup
#define JDS_ES_WAVES 4
#endif
constexpr int ES_WAVES = JDS_ES_WAVES;

// Append the L (< 32) bits of symL (left-aligned, zero below) to the pending
// word acc (n bits, left-aligned with zeros below: an append is one shift and
// one OR; right-aligned pending bits measured 0.2405 against 0.2385 ms); a
// completed word goes to the lane's LDS staging slot k (slots 64 words apart,
// so a wave's stores hit 64 banks), slots >= ES_SW to the segment's global
// area (same word-major layout: word k of lane l at (g * ES_MAXW + k) * 64 + l).
// a table symbol without its length field
__device__ __forceinline__ uint32_t es_code(uint32_t e) { return e & ~31u; }
struct EsStage {
  uint32_t* st;
  uint32_t* ov;
  int k = 0;
  // acc: the n pending bits left-aligned (the rest zero); symL clean (zero
  // below its L bits, 0 when L = 0)
  __device__ __forceinline__ void put(uint32_t symL, int L, uint32_t& acc, int& n) {
    const int t = n + L;
    const uint32_t w = acc | (symL >> n);
    if (t >= 32) {
      if (k < ES_SW) st[k * 64] = w; else ov[k * 64] = w;
      ++k;
      acc = __builtin_amdgcn_alignbit(symL, 0u, (uint32_t)n);  // the bits that did not fit (0 when n = 0)
    } else {
      acc = w;
    }
    n = t & 31;
  }
  __device__ __forceinline__ void store(uint32_t w) {
    if (k < ES_SW) st[k * 64] = w; else ov[k * 64] = w;
  }
};

// The AC walk, software-pipelined: e is position K's table entry, loaded
// while position K - 1 was appended; position K + 1's lookup (its run needs
// only whether K is nonzero) is issued before K's symbol is appended.
template <int K>
__device__ __forceinline__ void es_ac(const BlockRegs& r, int last, int& aor, const uint32_t* ac, uint32_t zrl,
                                      uint32_t& acc, int& n, EsStage& o, uint32_t e, int v, int sz, int& lastK) {
  if constexpr (K < ES_DENSE) {
    const int a = v < 0 ? -v : v;
    aor |= a;
    const int run = K - 1 - last;
    const int nlast = a ? K : last;
    uint32_t e1 = 0u;
    int v1 = 0, sz1 = 0;
    if constexpr (K + 1 < ES_DENSE) {
      v1 = coef_at<ZZC[K + 1]>(r);
      sz1 = es_size(v1 < 0 ? -v1 : v1);
      e1 = ac[((K - nlast) & 15) * ES_RS + sz1];
    }
    if (a && run >= 16) {  // rare: one ZRL code per 16 zeros first
      const int zl = (int)(zrl & 31u);
      for (int i = 0; i < (run >> 4); ++i) o.put(es_code(zrl), zl, acc, n);
    }
    const int L = (int)(e & 31u) + sz;
    const uint32_t mag = (uint32_t)(v + (v >> 31)) & ((1u << sz) - 1u);  // v, or v - 1 for v < 0, in sz bits
    o.put(es_code(e) | (mag << ((32 - L) & 31)), L, acc, n);
    es_ac<K + 1>(r, nlast, aor, ac, zrl, acc, n, o, e1, v1, sz1, lastK);
  } else {
    lastK = last;
  }
}

// Zigzag positions ES_DENSE .. 63 (mostly zero at every quality but the
// finest): their coefficients go to the lane's LDS column (int16, word-major
// across the wave) with a nonzero mask, and only the nonzero ones are coded,
// in order, by a per-lane loop (run lengths from the mask).
template <int K>
__device__ __forceinline__ void es_hi_stash(const BlockRegs& r, int16_t* cz, uint32_t& m) {
  if constexpr (K < 64) {
    const int v = coef_at<ZZC[K]>(r);
    cz[(K - ES_DENSE) * 64] = (int16_t)v;
    m |= (v != 0 ? 1u : 0u) << (K - ES_DENSE);
    es_hi_stash<K + 1>(r, cz, m);
  }
}

__device__ __forceinline__ void es_hi_code(const int16_t* cz, uint32_t m, int& last, int& aor, const uint32_t* ac,
                                           uint32_t zrl, uint32_t& acc, int& n, EsStage& o) {
  while (m) {
    const int b = __builtin_ctz(m);
    m &= m - 1u;
    const int K = ES_DENSE + b;
    const int v = cz[b * 64];
    const int a = v < 0 ? -v : v;
    aor |= a;
    const int sz = es_size(a);
    const int run = K - 1 - last;
    if (run >= 16) {  // one ZRL code per 16 zeros first
      const int zl = (int)(zrl & 31u);
      for (int i = 0; i < (run >> 4); ++i) o.put(es_code(zrl), zl, acc, n);
    }
    const uint32_t e = ac[(run & 15) * ES_RS + sz];
    const int L = (int)(e & 31u) + sz;
    const uint32_t mag = (uint32_t)(v + (v >> 31)) & ((1u << sz) - 1u);
    o.put(es_code(e) | (mag << ((32 - L) & 31)), L, acc, n);
    last = K;
  }
}

// One block: DC difference, AC walk, EOB, the partial word (left-aligned).
// Returns the bit count (32 per completed word + the pending bits); bd = not
// baseline-codable.
__device__ __forceinline__ uint32_t es_block(const BlockRegs& r, int diff, const EsTab& es, int cls, EsStage& o,
                                             bool& bd, int16_t* cz) {
  uint32_t acc = 0u;
  int n = 0;
  uint32_t mhi = 0u;
  if constexpr (ES_DENSE < 64) es_hi_stash<ES_DENSE>(r, cz, mhi);
  const int v1 = coef_at<ZZC[1]>(r);
  const int sz1 = es_size(v1 < 0 ? -v1 : v1);
  const uint32_t e1 = es.ac[cls][sz1];  // run 0
  const int da = diff < 0 ? -diff : diff;
  int ds = da ? 32 - __clz(da) : 0;
  bd = ds > 11;
  ds = ds > 11 ? 11 : ds;
  const uint32_t ed = es.dc[cls][ds];
  const int Ld = (int)(ed & 31u) + ds;
  const uint32_t md = (uint32_t)(diff + (diff >> 31)) & ((1u << ds) - 1u);
  o.put(es_code(ed) | (md << ((32 - Ld) & 31)), Ld, acc, n);
  int aor = 0, last = 0;
  es_ac<1>(r, 0, aor, es.ac[cls], es.zrl[cls], acc, n, o, e1, v1, sz1, last);
  if constexpr (ES_DENSE < 64) es_hi_code(cz, mhi, last, aor, es.ac[cls], es.zrl[cls], acc, n, o);
  const uint32_t eb = es.eob[cls];
  const int Le = last < 63 ? (int)(eb & 31u) : 0;  // EOB unless coefficient 63 is set
  o.put(Le ? es_code(eb) : 0u, Le, acc, n);
  bd |= aor > 1023;  // AC size > 10
  const uint32_t nb = 32u * (uint32_t)o.k + (uint32_t)n;
  o.store(acc);
  return nb;
}

// the scan's final word: 1-bits from the scan's end to its byte boundary;
// returns the number of the word's bytes that belong to the scan
__device__ __forceinline__ int es_pad(uint32_t& v, unsigned long long W1, unsigned long long widx) {
  const int used = (int)(W1 - 32ull * widx);  // 1..32
  const int pb = (8 - (used & 7)) & 7;
  if (pb) v |= ((1u << pb) - 1u) << (32 - used - pb);
  return (used + 7) >> 3;
}

// 0xFF bytes of a word as loaded from memory (byte j = bits 8j..8j+7), among its first nvb bytes
__device__ __forceinline__ int es_ff_mem(uint32_t x, int nvb) {
  const uint32_t y = ~x;
  const uint32_t hi = ~((((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) | 0x7F7F7F7Fu);  // bit 8j+7: byte j == 0xFF
  const uint32_t vm = nvb >= 4 ? 0x80808080u : (((1u << (8 * (nvb < 0 ? 0 : nvb))) - 1u) & 0x80808080u);
  return __popc(hi & vm);
}

__device__ __forceinline__ int es_ff(uint32_t v, int nbytes) {  // 0xFF bytes among the first nbytes (stream order)
  return es_ff_mem(__builtin_bswap32(v), nbytes);
}

// Placement of a segment's staged words at scan bit offset pre (lane bits at
// pre + excl): see "one pass" above.  st: the lane's LDS staging (slots <
// ES_SW), ov: its global words (slots >= ES_SW, or all slots when st is null).
// fuse (not the scan's last segment): tailx holds the next segment's bits that
// share this segment's final word, so that word is written whole here; Wn: the
// scan's end bit when the next segment ends in that word.  rs: the packed words
// the offsets count from (the scan's; a restart interval's own slot); report:
// the scan's last segment stores the scan's length (info, scan_bits).  SPAN:
// es_span().
template <int SPAN>
__device__ __forceinline__ void es_place(const EntGeo& e, const EsSeg& q, int g, int lane, bool valid, int nvalid,
                                         bool last_seg, uint32_t nb, uint32_t excl, unsigned long long pre,
                                         unsigned long long A, const uint32_t* st, const uint32_t* ov, int k,
                                         uint32_t* __restrict__ raw, unsigned long long* __restrict__ ffs,
                                         unsigned long long* __restrict__ info,
                                         unsigned long long* __restrict__ scan_bits, bool fuse, uint32_t tailx,
                                         unsigned long long Wn, uint32_t* __restrict__ rs, bool report) {
  const unsigned long long W1 = pre + A;
  auto stw = [&](int j) -> uint32_t { return j >= k ? 0u : ((st == nullptr || j >= ES_SW) ? ov[j * 64] : st[j * 64]); };
  const unsigned long long o = pre + excl;  // the lane's first bit in the scan
  const int sh = (int)(o & 31ull);
  const unsigned long long hw = o >> 5, tw = (o + nb - 1ull) >> 5;
  const bool single = hw == tw;
  const uint32_t s0 = stw(0);
  const uint32_t hv = s0 >> sh;
  // the next lane starts inside this lane's tail word
  // (fuse: lane 63's "next lane" is the next segment, whose bits are tailx)
  const bool c = valid && ((o + nb) & 31ull) != 0ull && (lane + 1 < nvalid || fuse);
  // X = this lane's head word bits | those of the following lanes that share it
  uint32_t X = valid ? hv : 0u;
  int F = (valid && single && c) ? 1 : 0;
  if (fuse && lane == 63 && F) {
    X |= tailx;
    F = 0;
  }
  // (every block costs >= 4 bits, so at most 7 lanes in a row lie inside one
  // word and share the next lane's word: spans of 8 lanes suffice; the host
  // model fails with spans of 4.  Optimised tables: >= 2 bits, 15 lanes.)
  {  // X_l = own_l | (F_l ? X_{l+1} : 0), one lane further per DPP wave shift (lane 63 never chains)
    // (a mask, not a select: the shifts must run with every lane active, and
    // the compiler turns a select into a branch around them)
    const uint32_t own = X, fm = 0u - (uint32_t)F;
#pragma unroll
    for (int it = 0; it < SPAN; ++it) X = own | (wave_shl1(X) & fm);
  }
  const uint32_t X1 = wave_shl1(X);
  const uint32_t in_tail = c ? ((fuse && lane == 63) ? tailx : X1) : 0u;
  // word indices within the scan fit 32 bits (< 2^28 words)
  const uint32_t wlast = (uint32_t)((W1 - 1ull) >> 5);
  const bool open_end = !fuse && !last_seg && (W1 & 31ull);
  const unsigned long long Wend = last_seg ? W1 : Wn;  // the scan ends in word wlast (0: it does not)
  const uint32_t padw = Wend ? wlast : 0xFFFFFFFFu;     // the word that takes the pad bits
  const uint32_t skipw = open_end ? wlast : 0xFFFFFFFFu;  // the word the next segment counts
  int ffc = 0;
  auto put_word = [&](uint32_t widx, uint32_t v) {
    int nb4 = 4;
    if (widx == padw) nb4 = es_pad(v, Wend, widx);
    rs[widx] = __builtin_bswap32(v);  // byte 0 of the stream first
    if (widx != skipw) ffc += es_ff(v, nb4);
  };
  if (valid) {
    const bool own_head = sh == 0;
    const int nout = (int)(tw - hw);
    const uint32_t hw32 = (uint32_t)hw, tw32 = (uint32_t)tw;
    if (own_head && !single) put_word(hw32, hv);
    uint32_t prev = s0;
    int j = 1;
    for (; j + 3 < nout; j += 4) {  // four staged words requested before any is used
      const uint32_t c0 = stw(j), c1 = stw(j + 1), c2 = stw(j + 2), c3 = stw(j + 3);
      put_word(hw32 + j, __builtin_amdgcn_alignbit(prev, c0, (uint32_t)sh));
      put_word(hw32 + j + 1, __builtin_amdgcn_alignbit(c0, c1, (uint32_t)sh));
      put_word(hw32 + j + 2, __builtin_amdgcn_alignbit(c1, c2, (uint32_t)sh));
      put_word(hw32 + j + 3, __builtin_amdgcn_alignbit(c2, c3, (uint32_t)sh));
      prev = c3;
    }
    for (; j < nout; ++j) {
      const uint32_t cur = stw(j);
      put_word(hw32 + j, __builtin_amdgcn_alignbit(prev, cur, (uint32_t)sh));
      prev = cur;
    }
    const uint32_t tv = single ? hv : __builtin_amdgcn_alignbit(prev, stw(nout), (uint32_t)sh);
    if (!single || own_head) put_word(tw32, tv | in_tail);
  }
  ffc = (int)wave_sum((uint32_t)ffc);
  if (lane == 0) {
    ffs[g] = (unsigned long long)ffc;
    if (last_seg && report) {
      info[2 * (q.f * 3 + q.s)] = 0ull;
      info[2 * (q.f * 3 + q.s) + 1] = W1;
      if (scan_bits) scan_bits[q.f * 3 + q.s] = W1;
    }
  }
}

// scans of at most this many segments sum their earlier totals themselves
// (k_ent_place; measurements there)
constexpr int ES_SELF_MAX = 512;

// bytes of packed scan per round of em_copy (16 B per lane)
constexpr int EM_CHUNK = 1024;

// Stuffed copy of bytes [b0, b1) of the packed words w to dst by one wave (sb:
// the wave's LDS buffer); returns the end of what it wrote.
__device__ __forceinline__ uint8_t* em_copy(const uint32_t* __restrict__ w, unsigned long long b0,
                                            unsigned long long b1, uint8_t* dst, uint32_t* sb, int lane) {
  uint8_t* lb = reinterpret_cast<uint8_t*>(sb);
  for (unsigned long long i0 = b0; i0 < b1; i0 += EM_CHUNK) {
    // lane l takes the chunk's dwords l, l + 64, l + 128, l + 192: coalesced
    // loads, and a wave's byte stores land on consecutive LDS words (16 B per
    // lane put lanes 16 apart on one bank)
    uint32_t x[4];
    int nvk[4], lk[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned long long i = i0 + 4 * (64 * k + lane);
      nvk[k] = i < b1 ? (b1 - i < 4 ? (int)(b1 - i) : 4) : 0;
      x[k] = nvk[k] ? w[i >> 2] : 0u;
      lk[k] = nvk[k] + es_ff_mem(x[k], nvk[k]);  // <= 8
    }
    // two packed scans (16-bit fields: a field's wave sum is <= 512)
    const uint32_t pa = (uint32_t)lk[0] | ((uint32_t)lk[1] << 16), pb = (uint32_t)lk[2] | ((uint32_t)lk[3] << 16);
    const uint32_t ia = wave_incl_sum(pa, lane), ib = wave_incl_sum(pb, lane);
    const uint32_t ta = lane63(ia), tb = lane63(ib);
    const uint32_t ea = ia - pa, eb = ib - pb;
    const int t0 = (int)(ta & 0xFFFFu), t1 = (int)(ta >> 16), t2 = (int)(tb & 0xFFFFu), t3 = (int)(tb >> 16);
    const int tot = t0 + t1 + t2 + t3;
    const int sh0 = (int)((uintptr_t)dst & 3u);  // LDS byte sh0 <-> dst[0]
    const int pk[4] = {sh0 + (int)(ea & 0xFFFFu), sh0 + t0 + (int)(ea >> 16), sh0 + t0 + t1 + (int)(eb & 0xFFFFu),
                       sh0 + t0 + t1 + t2 + (int)(eb >> 16)};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int p = pk[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < nvk[k]) {
          const uint8_t b = (uint8_t)(x[k] >> (8 * j));
          lb[p++] = b;
          if (b == 0xFF) lb[p++] = 0x00;
        }
      }
    }
    __builtin_amdgcn_wave_barrier();  // one wave: its LDS operations execute in order
    asm volatile("" ::: "memory");
    // out: global bytes dst[0 .. tot) <- LDS bytes [sh0, sh0 + tot); dword d covers LDS [4d, 4d + 4)
    uint8_t* a0 = dst - sh0;  // 4-byte aligned
    const int nd = (sh0 + tot + 3) >> 2;
    for (int d = lane; d < nd; d += 64) {
      const int lo = 4 * d, hi = 4 * d + 4;
      if (lo >= sh0 && hi <= sh0 + tot) {
        *reinterpret_cast<uint32_t*>(a0 + lo) = sb[d];
      } else {
        for (int c = lo; c < hi; ++c)
          if (c >= sh0 && c < sh0 + tot) a0[c] = lb[c];
      }
    }
    __builtin_amdgcn_wave_barrier();  // the buffer is reused by the next iteration
    asm volatile("" ::: "memory");
    dst += tot;
  }
  return dst;
}

// The symbol histogram's AC walk (k_ent_hist, k_mcu_hist).  bins: the lane's copy of
// its wave's [16 DC categories + 256 AC symbols] counters, bin i at bins[i * EH_COPIES].
constexpr int EH_ZRL = 16 + 0xF0, EH_EOB = 16 + 0x00;
// zigzag positions K..63 of the lane's block: one count per non-zero
// coefficient ((run & 15) << 4 | size, size clamped like the coder's), one ZRL
// count per 16 zeros before it
template <int K, int EH_COPIES>
__device__ __forceinline__ void eh_ac(const BlockRegs& r, int last, int& aor, uint32_t* bins, int& lastK) {
  if constexpr (K < 64) {
    const int v = coef_at<ZZC[K]>(r);
    const int a = v < 0 ? -v : v;
    if (a) {
      const int run = K - 1 - last;
      if (run >= 16) atomicAdd(&bins[EH_ZRL * EH_COPIES], (uint32_t)(run >> 4));
      atomicAdd(&bins[(16 + (((run & 15) << 4) | es_size(a))) * EH_COPIES], 1u);
      aor |= a;
      last = K;
    }
    eh_ac<K + 1, EH_COPIES>(r, last, aor, bins, lastK);
  } else {
    lastK = last;
  }
}

}  // namespace jds
